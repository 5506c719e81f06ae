// Box plumbing of multi-scale / flip test-time augmentation, device-resident (the reference runs it per frame on the host side of
// the tensors: one NMS call with a host read per frame, mmdet/core/post_processing/merge_augs.py:8-70 over
// mmdet/core/bbox/transforms.py:114-146, driven by HNMBRCNN.forward_feat_aug / aug_test_bboxes, hnmb_rcnn.py:104-180, 640-698):
//
//   * merge_aug_proposals for all T frames of a window  <- merge_augs.py:8-44 (bbox_mapping_back, cat, nms, sort, [:max_num])
//   * bbox_mapping + bbox2roi for every augmentation     <- transforms.py:131-136,149-168 as hnmb_rcnn.py:645-651 calls them
//   * merge_aug_bboxes                                   <- merge_augs.py:47-70
//
// Arithmetic: un-flip / flip are `img_w - x - 1` evaluated left to right, the way back divides by scale_factor (a true division,
// as hvr_det_decode's rescale), the way forward multiplies; this file is compiled without contraction so that `img_w - x * s - 1`
// keeps the reference's two roundings.  No kernel here reads anything back to the host.
#include "common.h"
#include "nms_dev.h"

namespace hvr {

constexpr int TTA_MAX_AUGS = 16;

struct TtaAugs {
  int A;
  float img_w[TTA_MAX_AUGS], scale[TTA_MAX_AUGS];
  int flip[TTA_MAX_AUGS];
};

// bbox_mapping_back (transforms.py:139-143) of one box
__device__ __forceinline__ float4 tta_map_back(float x1, float y1, float x2, float y2, float img_w, float scale, int flip) {
  float a = x1, b = x2;
  if (flip) {
    a = img_w - x2 - 1.f;
    b = img_w - x1 - 1.f;
  }
  return make_float4(a / scale, y1 / scale, b / scale, y2 / scale);
}

// One workgroup of 1024 threads per frame.
//   1. the valid rows of every augmentation (row < counts[a][t]) get their concatenated index (augmentation order) and are sorted
//      by (score descending, concatenated index ascending) -- the order in which greedy NMS visits them and, since survivors are met
//      in that order, also the order of the output;
//   2. the boxes are mapped back to the original image and laid out in the LDS in sorted order (over the sort buffer);
//   3. greedy NMS with IoU >= thr (nms_cpu.cpp:5-59): the next box that is not yet suppressed survives, the whole workgroup marks
//      what it suppresses behind it (one ballot per 64 boxes), until max_num survivors are found or the boxes run out;
//   4. survivor k -> out[t][k], zeros behind the count.
// ws: [T][np2] sorted composites (score key << 32 | 0xffffffff - concatenated index), so that step 4 finds a survivor's source row.
__global__ __launch_bounds__(1024) void tta_merge_proposals_kernel(const float* __restrict__ props, const int* __restrict__ counts,
                                                                   TtaAugs au, int T, int mx, int np2, float thr, int max_num,
                                                                   float* __restrict__ out, int* __restrict__ out_counts,
                                                                   unsigned long long* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int A = au.A;
  unsigned long long* sortbuf = reinterpret_cast<unsigned long long*>(smem);          // [np2]          (steps 1-2)
  float4* box = reinterpret_cast<float4*>(smem);                                        // [np2]          (steps 2-4, over sortbuf)
  unsigned long long* removed = reinterpret_cast<unsigned long long*>(smem + (size_t)np2 * 16);  // [max(np2 / 64, 1)]
  const int nw = np2 >= 64 ? np2 >> 6 : 1;
  unsigned short* kall = reinterpret_cast<unsigned short*>(removed + nw);             // [max_num] survivors' sorted positions
  __shared__ int pre[TTA_MAX_AUGS + 1];
  if (tid == 0) {
    int s = 0;
    for (int a = 0; a < A; ++a) {
      pre[a] = s;
      const int c = counts[a * T + t];
      s += c < 0 ? 0 : (c > mx ? mx : c);
    }
    for (int a = A; a <= TTA_MAX_AUGS; ++a) pre[a] = s;
  }
  __syncthreads();
  const int n = pre[A];
  unsigned long long* wst = ws + (size_t)t * np2;

  // 1. composites of the valid rows, pads 0
  for (int i = tid; i < np2; i += blockDim.x) sortbuf[i] = 0ull;
  __syncthreads();
  for (int a = 0; a < A; ++a) {
    const int c = pre[a + 1] - pre[a];
    const float* p = props + ((size_t)a * T + t) * mx * 5;
    for (int r = tid; r < c; r += blockDim.x) {
      const uint32_t ci = (uint32_t)(pre[a] + r);
      sortbuf[ci] = ((unsigned long long)float_key(p[r * 5 + 4]) << 32) | (0xffffffffu - ci);
    }
  }
  __syncthreads();
  block_sort_desc_u64(sortbuf, np2);
  __syncthreads();

  // 2. sorted composites -> registers -> mapped boxes in sorted order
  unsigned long long ent[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int i = m * 1024 + tid;
    ent[m] = i < np2 ? sortbuf[i] : 0ull;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int i = m * 1024 + tid;
    if (i >= np2) continue;
    wst[i] = ent[m];
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
      const int ci = (int)(0xffffffffu - (uint32_t)ent[m]);
      int a = 0;
      while (a + 1 < A && ci >= pre[a + 1]) ++a;
      const float* p = props + (((size_t)a * T + t) * mx + (ci - pre[a])) * 5;
      b = tta_map_back(p[0], p[1], p[2], p[3], au.img_w[a], au.scale[a], au.flip[a]);
    }
    box[i] = b;
  }
  for (int i = tid; i < nw; i += blockDim.x) removed[i] = 0ull;
  __syncthreads();

  // 3. greedy sweep: every thread walks the same positions (the suppression words are only written between barriers and a
  //    thread that runs ahead only sets bits behind the box all threads are about to pick)
  const float band_k = iou_band_k(thr);
  int nkept = 0, i = 0;
  while (i < n && nkept < max_num) {
    const unsigned long long word = removed[i >> 6];
    const int base = i & ~63, cnt = min(64, n - base);
    const unsigned long long valid = cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull);
    const unsigned long long cand = ~word & valid & ~((1ull << (i & 63)) - 1ull);
    if (!cand) {
      i = base + 64;
      continue;
    }
    i = base + __builtin_ctzll(cand);
    if (tid == 0) kall[nkept] = (unsigned short)i;
    ++nkept;
    if (nkept < max_num) {
      const float4 bi = box[i];
      const float ai = box_area_plus1(bi);
      for (int j = ((i + 1) & ~63) + tid; j < ((n + 63) & ~63); j += blockDim.x) {   // whole waves stay together for the ballot
        bool hit = false;
        if (j > i && j < n) {
          const float4 bj = box[j];
          hit = box_iou_hits(bi, ai, bj, box_area_plus1(bj), thr, band_k, 1);
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0 && m) atomicOr(&removed[j >> 6], m);
      }
    }
    __syncthreads();
    ++i;
  }
  __syncthreads();

  // 4. survivors in sweep order = descending score, ties by lower concatenated index
  for (int k = tid; k < max_num; k += blockDim.x) {
    float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (k < nkept) {
      const int pos = (int)kall[k];
      const float4 b = box[pos];
      const uint32_t key = (uint32_t)(wst[pos] >> 32);
      const uint32_t u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;   // float_key inverted
      o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = __uint_as_float(u);
    }
    float* dst = out + ((size_t)t * max_num + k) * 5;
#pragma unroll
    for (int e = 0; e < 5; ++e) dst[e] = o[e];
  }
  if (tid == 0) out_counts[t] = nkept;
}

// bbox_mapping (transforms.py:131-136) + bbox2roi: rois[a][t * max_num + r] = (t, merged[t][r] * scale_a, flipped in aug a's width)
__global__ __launch_bounds__(256) void tta_map_rois_kernel(const float* __restrict__ merged, TtaAugs au, int rows, int max_num,
                                                           float* __restrict__ rois) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y;
  if (r >= rows) return;
  const float* p = merged + (size_t)r * 5;
  const float s = au.scale[a], w = au.img_w[a];
  float x1 = p[0] * s, y1 = p[1] * s, x2 = p[2] * s, y2 = p[3] * s;
  if (au.flip[a]) {
    const float f1 = w - x2 - 1.f, f2 = w - x1 - 1.f;
    x1 = f1;
    x2 = f2;
  }
  float* o = rois + ((size_t)a * rows + r) * 5;
  o[0] = (float)(r / max_num);
  o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
}

// merge_aug_bboxes (merge_augs.py:47-70): boxes mapped back and averaged over the augmentations, scores averaged; sums in
// augmentation order, one division by A.  One thread per output element (4 box coordinates, then ncls scores per row).
__global__ __launch_bounds__(256) void tta_merge_dets_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             TtaAugs au, int R, int ncls, float* __restrict__ out_boxes,
                                                             float* __restrict__ out_scores) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, per = 4 + ncls;
  if (e >= R * per) return;
  const int r = e / per, c = e % per, A = au.A;
  float acc = 0.f;
  if (c < 4) {
    for (int a = 0; a < A; ++a) {
      const float* b = boxes + ((size_t)a * R + r) * 4;
      float v = b[c];
      if (au.flip[a] && !(c & 1)) v = au.img_w[a] - b[2 - c] - 1.f;   // x1 <- w - x2 - 1, x2 <- w - x1 - 1
      v = v / au.scale[a];
      acc = a == 0 ? v : acc + v;
    }
    out_boxes[(size_t)r * 4 + c] = acc / (float)A;
  } else {
    for (int a = 0; a < A; ++a) {
      const float v = scores[((size_t)a * R + r) * ncls + (c - 4)];
      acc = a == 0 ? v : acc + v;
    }
    out_scores[(size_t)r * ncls + (c - 4)] = acc / (float)A;
  }
}

static int tta_np2(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}

size_t tta_merge_proposals_workspace_bytes(int A, int T, int mx) { return (size_t)T * tta_np2(A * mx) * 8 + 256; }

static TtaAugs tta_augs(int A, const float* img_w, const float* scale, const int* flip) {
  TtaAugs au;
  au.A = A;
  for (int a = 0; a < TTA_MAX_AUGS; ++a) {
    au.img_w[a] = a < A ? img_w[a] : 0.f;
    au.scale[a] = a < A ? scale[a] : 1.f;
    au.flip[a] = a < A ? (flip[a] != 0) : 0;
  }
  return au;
}

hipError_t run_tta_merge_proposals(const float* props, const int* counts, int A, int T, int mx, const float* img_w, const float* scale,
                                   const int* flip, float thr, int max_num, float* out, int* out_counts, void* ws, hipStream_t s) {
  if (A <= 0 || A > TTA_MAX_AUGS || T <= 0 || mx <= 0 || (long)A * mx > 8192 || max_num <= 0 || max_num > 4096) return hipErrorInvalidValue;
  const int np2 = tta_np2(A * mx);
  static std::atomic<unsigned> attr_dev{0};   // (the attribute is per device)
  per_device_once(attr_dev, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(tta_merge_proposals_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              8192 * 16 + 128 * 8 + 4096 * 2);
  });
  const size_t lds = (size_t)np2 * 16 + (size_t)(np2 >> 6) * 8 + (size_t)max_num * 2;
  hipLaunchKernelGGL(tta_merge_proposals_kernel, dim3(T), dim3(1024), lds, s, props, counts, tta_augs(A, img_w, scale, flip), T, mx, np2,
                     thr, max_num, out, out_counts, (unsigned long long*)ws);
  return hipGetLastError();
}

hipError_t run_tta_map_rois(const float* merged, int A, int T, int max_num, const float* img_w, const float* scale, const int* flip,
                            float* rois, hipStream_t s) {
  if (A <= 0 || A > TTA_MAX_AUGS || T <= 0 || max_num <= 0) return hipErrorInvalidValue;
  const int rows = T * max_num;
  hipLaunchKernelGGL(tta_map_rois_kernel, dim3((rows + 255) / 256, A), dim3(256), 0, s, merged, tta_augs(A, img_w, scale, flip), rows,
                     max_num, rois);
  return hipGetLastError();
}

hipError_t run_tta_merge_dets(const float* boxes, const float* scores, int A, int R, int ncls, const float* img_w, const float* scale,
                              const int* flip, float* out_boxes, float* out_scores, hipStream_t s) {
  if (A <= 0 || A > TTA_MAX_AUGS || R <= 0 || ncls <= 0) return hipErrorInvalidValue;
  const int total = R * (4 + ncls);
  hipLaunchKernelGGL(tta_merge_dets_kernel, dim3((total + 255) / 256), dim3(256), 0, s, boxes, scores, tta_augs(A, img_w, scale, flip), R,
                     ncls, out_boxes, out_scores);
  return hipGetLastError();
}

}  // namespace hvr
