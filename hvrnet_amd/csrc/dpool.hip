// Deformable (position-sensitive) RoI pooling, forward only: the pooling half of DCN v1 / v2.
// Replaces mmdet/ops/dcn/src/deform_pool_cuda_kernel.cu:30-50 (bilinear rule) and :52-140 (DeformablePSROIPoolForwardKernel).
// Same arithmetic per sample in the same order (the rule is stated in include/hvr_hip.h); RoIAlign's layout and parallelisation
// (roi_align.hip), not the reference's one-thread-per-output flat index:
//   * one workgroup per RoI, all frames of a call in ONE launch (the roi's batch index selects the frame);
//   * the map is physical NHWC: lanes run along channels, 16 bytes of channels per lane, the bins are spread over the remaining
//     lane groups; stores are whole contiguous pieces of out [roi][bin][Cout];
//   * a sample's validity, cells and weights factor per axis: the spp columns are resolved once per bin, a row once per row of
//     samples, and the 4 * spp corner loads of a row are issued back to back on clamped (always in-bounds) addresses.  A
//     skipped sample's loads still happen; its products are not accumulated (a select, no data-dependent branch between loads);
//   * no run-time integer division on the per-sample path: two per thread, one per bin (ph, pw), one per (bin, lane) for the
//     class of the offset.
// group_size > 1 (position-sensitive maps) takes the one-channel-per-lane instance: the lane's channel is
// (ct * gs + gh) * gs + gw, consecutive ct are gs * gs channels apart.  So do shapes whose classes split a 16-byte piece.
// Built with -ffp-contract=off (build.sh): every product and sum is rounded on its own, which is what the f64 statement of the
// tests counts (tests/dpool_refs.py).  The mask is 1 / (1 + expf(-logit)) with the documented-accuracy expf and a correctly
// rounded add and divide, as in dcn.hip.
#include "common.h"

namespace hvr {

struct DpoolShape {
  int B, H, W, C, Cout, P, spp, gs, ps, ncls;
  long ldt, ldm;
  float scale, trans_std;
};

// one axis of a sample: skipped outside [-0.5, size - 0.5]; else clamped to the map's edge, floor / ceil cells, distance to floor
struct DpAxis { int lo, hi; float d; bool ok; };
__device__ __forceinline__ DpAxis dp_axis(int size, float v) {
  DpAxis t;
  t.ok = !(v < -0.5f || v > (float)size - 0.5f);
  const float c = fminf(fmaxf(v, 0.f), (float)(size - 1));   // (NaN -> 0: the address stays in bounds)
  const float fl = floorf(c);
  t.lo = (int)fl;
  t.hi = (int)ceilf(c);
  t.d = c - fl;
  return t;
}

// CV channels of one corner as loaded (CV > 1: one 16-byte piece; CV == 1: one element, converted)
template <typename T, int CV> struct DpRaw { uint4 a; };
template <typename T> struct DpRaw<T, 1> { float a; };

template <typename T, int CV> __device__ __forceinline__ DpRaw<T, CV> dp_load(const T* p) {
  DpRaw<T, CV> r;
  if constexpr (CV == 1) r.a = ElemTraits<T>::load(p);
  else r.a = *reinterpret_cast<const uint4*>(p);
  return r;
}
template <typename T, int CV> __device__ __forceinline__ void dp_unpack(const DpRaw<T, CV>& r, float* f) {
  if constexpr (CV == 1) {
    f[0] = r.a;
  } else if constexpr (std::is_same<T, float>::value) {
    f[0] = __uint_as_float(r.a.x); f[1] = __uint_as_float(r.a.y); f[2] = __uint_as_float(r.a.z); f[3] = __uint_as_float(r.a.w);
  } else {
    unpack2<T>(r.a.x, f[0], f[1]); unpack2<T>(r.a.y, f[2], f[3]); unpack2<T>(r.a.z, f[4], f[5]); unpack2<T>(r.a.w, f[6], f[7]);
  }
}
template <typename T, int CV> __device__ __forceinline__ void dp_store(T* p, const float* f) {
  if constexpr (CV == 1) {
    ElemTraits<T>::store(p, f[0]);
  } else if constexpr (std::is_same<T, float>::value) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  } else {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
  }
}

// sum += the bilinear value of one sample, the four products in the reference's order (deform_pool_cuda_kernel.cu:48)
template <typename T, int CV>
__device__ __forceinline__ void dp_accumulate(float* acc, bool ok, float dx, float dy, const DpRaw<T, CV>& r11, const DpRaw<T, CV>& r12,
                                              const DpRaw<T, CV>& r21, const DpRaw<T, CV>& r22) {
  float v11[CV], v12[CV], v21[CV], v22[CV];
  dp_unpack<T, CV>(r11, v11); dp_unpack<T, CV>(r12, v12); dp_unpack<T, CV>(r21, v21); dp_unpack<T, CV>(r22, v22);
  const float omx = 1.f - dx, omy = 1.f - dy;
  const float w11 = omx * omy, w12 = omx * dy, w21 = dx * omy, w22 = dx * dy;
#pragma unroll
  for (int e = 0; e < CV; ++e) {
    const float val = w11 * v11[e] + w12 * v12[e] + w21 * v21[e] + w22 * v22[e];
    acc[e] = ok ? acc[e] + val : acc[e];
  }
}

// SPP > 0: sample_per_part known at compile time (a row of samples in flight); SPP == 0: any sample_per_part, one sample in flight
template <typename T, int CV, int SPP>
__global__ __launch_bounds__(256) void deform_roi_pool_kernel(const T* __restrict__ feat, const float* __restrict__ rois,
                                                              const float* __restrict__ trans, const float* __restrict__ mask_logit,
                                                              T* __restrict__ out, const DpoolShape s) {
  const int k = blockIdx.x;
  const int lanes_c = s.Cout / CV;                       // 16-byte pieces (CV == 1: channels) of one output bin
  const int lanes_used = lanes_c < 256 ? lanes_c : 256;  // threads along channels
  const int groups = 256 / lanes_used;                   // bins in flight
  const int grp = (int)threadIdx.x / lanes_used, cl0 = (int)threadIdx.x - grp * lanes_used;
  if (grp >= groups) return;
  const int P = s.P, H = s.H, W = s.W, C = s.C, ps = s.ps, gs = s.gs;
  const int spp = SPP > 0 ? SPP : s.spp;
  const float* roi = rois + (long)k * 5;
  const int b = min(max((int)roi[0], 0), s.B - 1);       // (a batch index outside the call's frames is clamped: no read outside the map)
  const float start_w = roundf(roi[1]) * s.scale - 0.5f;
  const float start_h = roundf(roi[2]) * s.scale - 0.5f;
  const float end_w = (roundf(roi[3]) + 1.f) * s.scale - 0.5f;
  const float end_h = (roundf(roi[4]) + 1.f) * s.scale - 0.5f;
  const float roi_w = fmaxf(end_w - start_w, 0.1f), roi_h = fmaxf(end_h - start_h, 0.1f);
  const float bin_w = roi_w / (float)P, bin_h = roi_h / (float)P;
  const float sub_w = bin_w / (float)spp, sub_h = bin_h / (float)spp;
  const int cpc = s.Cout / s.ncls;                       // output channels of one class
  const T* fb = feat + (long)b * H * W * C;
  for (int bin = grp; bin < P * P; bin += groups) {
    const int ph = bin / P, pw = bin - ph * P;
    const int part_h = min(max((int)floorf((float)ph / (float)P * (float)ps), 0), ps - 1);
    const int part_w = min(max((int)floorf((float)pw / (float)P * (float)ps), 0), ps - 1);
    const int gw = min(max((int)floorf((float)pw * (float)gs / (float)P), 0), gs - 1);
    const int gh = min(max((int)floorf((float)ph * (float)gs / (float)P), 0), gs - 1);
    const float wstart0 = (float)pw * bin_w + start_w, hstart0 = (float)ph * bin_h + start_h;
    float mask = 1.f;
    if (mask_logit) mask = 1.f / (1.f + expf(-mask_logit[(long)k * s.ldm + bin]));
    for (int cl = cl0; cl < lanes_c; cl += lanes_used) {
      const int ct = cl * CV;                            // first output channel of this lane
      float tx = 0.f, ty = 0.f;
      if (trans) {
        const int cls = ct / cpc;
        const float* t = trans + (long)k * s.ldt + ((long)(cls * 2) * ps + part_h) * ps + part_w;
        tx = t[0] * s.trans_std;
        ty = t[ps * ps] * s.trans_std;
      }
      const float wstart = wstart0 + tx * roi_w, hstart = hstart0 + ty * roi_h;
      const T* fc = fb + (CV == 1 ? (ct * gs + gh) * gs + gw : ct);
      float acc[CV];
#pragma unroll
      for (int e = 0; e < CV; ++e) acc[e] = 0.f;
      int count = 0;
      if constexpr (SPP > 0) {
        DpAxis ax[SPP];
        int nw = 0;
#pragma unroll
        for (int iw = 0; iw < SPP; ++iw) {
          ax[iw] = dp_axis(W, wstart + (float)iw * sub_w);
          nw += ax[iw].ok ? 1 : 0;
        }
#pragma unroll
        for (int ih = 0; ih < SPP; ++ih) {
          const DpAxis ay = dp_axis(H, hstart + (float)ih * sub_h);
          const T* rl = fc + (long)ay.lo * W * C;
          const T* rh = fc + (long)ay.hi * W * C;
          DpRaw<T, CV> r[SPP][4];
#pragma unroll
          for (int iw = 0; iw < SPP; ++iw) {
            r[iw][0] = dp_load<T, CV>(rl + (long)ax[iw].lo * C);   // [yl][xl]
            r[iw][1] = dp_load<T, CV>(rh + (long)ax[iw].lo * C);   // [yh][xl]
            r[iw][2] = dp_load<T, CV>(rl + (long)ax[iw].hi * C);   // [yl][xh]
            r[iw][3] = dp_load<T, CV>(rh + (long)ax[iw].hi * C);   // [yh][xh]
          }
#pragma unroll
          for (int iw = 0; iw < SPP; ++iw)
            dp_accumulate<T, CV>(acc, ay.ok && ax[iw].ok, ax[iw].d, ay.d, r[iw][0], r[iw][1], r[iw][2], r[iw][3]);
          count += ay.ok ? nw : 0;
        }
      } else {
        for (int ih = 0; ih < spp; ++ih) {
          const DpAxis ay = dp_axis(H, hstart + (float)ih * sub_h);
          const T* rl = fc + (long)ay.lo * W * C;
          const T* rh = fc + (long)ay.hi * W * C;
          for (int iw = 0; iw < spp; ++iw) {
            const DpAxis ax = dp_axis(W, wstart + (float)iw * sub_w);
            const DpRaw<T, CV> r11 = dp_load<T, CV>(rl + (long)ax.lo * C), r12 = dp_load<T, CV>(rh + (long)ax.lo * C);
            const DpRaw<T, CV> r21 = dp_load<T, CV>(rl + (long)ax.hi * C), r22 = dp_load<T, CV>(rh + (long)ax.hi * C);
            const bool ok = ay.ok && ax.ok;
            dp_accumulate<T, CV>(acc, ok, ax.d, ay.d, r11, r12, r21, r22);
            count += ok ? 1 : 0;
          }
        }
      }
      const float cnt = (float)count;
#pragma unroll
      for (int e = 0; e < CV; ++e) {
        float v = count == 0 ? 0.f : acc[e] / cnt;
        if (mask_logit) v = v * mask;
        acc[e] = v;
      }
      dp_store<T, CV>(out + ((long)k * P * P + bin) * s.Cout + ct, acc);
    }
  }
}

template <typename T, int CV>
static hipError_t launch_deform_roi_pool_cv(const void* feat, const float* rois, const float* trans, const float* mask, void* out, const DpoolShape& s,
                                            int K, hipStream_t st) {
  if (s.spp == 4)
    hipLaunchKernelGGL((deform_roi_pool_kernel<T, CV, 4>), dim3(K), dim3(256), 0, st, (const T*)feat, rois, trans, mask, (T*)out, s);
  else if (s.spp == 2)
    hipLaunchKernelGGL((deform_roi_pool_kernel<T, CV, 2>), dim3(K), dim3(256), 0, st, (const T*)feat, rois, trans, mask, (T*)out, s);
  else
    hipLaunchKernelGGL((deform_roi_pool_kernel<T, CV, 0>), dim3(K), dim3(256), 0, st, (const T*)feat, rois, trans, mask, (T*)out, s);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_deform_roi_pool(const void* feat, const float* rois, const float* trans, const float* mask, void* out, const DpoolShape& s,
                                         int K, hipStream_t st) {
  constexpr int CV = 16 / (int)sizeof(T);
  const bool al16 = ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  // 16 bytes per lane: the lane's channels are consecutive in the map (gs == 1), whole pieces per bin, one class per piece
  if (s.gs == 1 && s.Cout % CV == 0 && (s.Cout / s.ncls) % CV == 0 && al16)
    return launch_deform_roi_pool_cv<T, CV>(feat, rois, trans, mask, out, s, K, st);
  return launch_deform_roi_pool_cv<T, 1>(feat, rois, trans, mask, out, s, K, st);
}

// shapes are validated by the C ABI (capi.hip: hvr_deform_roi_pool_fwd)
hipError_t run_deform_roi_pool(const void* feat, const float* rois, const float* trans, const float* mask, void* out, int B, int H, int W, int C,
                               int K, int P, int Cout, int gs, int ps, int ncls, int spp, float scale, float trans_std, long ldt, long ldm,
                               int dtype, hipStream_t st) {
  if (K == 0) return hipSuccess;
  DpoolShape s;
  s.B = B; s.H = H; s.W = W; s.C = C; s.Cout = Cout; s.P = P; s.spp = spp; s.gs = gs; s.ps = ps; s.ncls = ncls;
  s.ldt = ldt; s.ldm = ldm; s.scale = scale; s.trans_std = trans_std;
  if (dtype == DT_BF16) return launch_deform_roi_pool<bf16_t>(feat, rois, trans, mask, out, s, K, st);
  if (dtype == DT_F16) return launch_deform_roi_pool<f16_t>(feat, rois, trans, mask, out, s, K, st);
  if (dtype == DT_F32) return launch_deform_roi_pool<float>(feat, rois, trans, mask, out, s, K, st);
  return hipErrorInvalidValue;
}

}  // namespace hvr
