// Body fragment, included INSIDE a kernel (no include guard: it is statements, not declarations): the bins of one RoI in the path's own
// configuration (sample_num = 2, 2-byte elements, 16 B of channels per lane): the same arithmetic in the same order as roi_align_bins.h,
// with the four sample points of a bin resolved first and their 16 gathers issued back to back -- the generic body's data-dependent
// `continue` keeps the compiler from overlapping one sample's loads with the next sample's (the kernel is latency-bound: 4 500
// workgroups of short dependent gather chains).  A sample outside the map keeps the reference's "skip" (roi_align_kernel.cu:29-35): its
// taps read pixel (0, 0) and are not accumulated.  In scope at the point of inclusion: the type T (bf16_t / f16_t) and
//   const T* feat; const float* roi (the RoI's five floats); T* out; int k, C, H, W, PH, PW; float spatial_scale.
  const int lanes_c = C / 8;
  const int groups = blockDim.x / lanes_c;
  const int cl = threadIdx.x % lanes_c, grp = threadIdx.x / lanes_c;
  if (grp >= groups) return;
  const RoiGeom g = roi_geom(roi, spatial_scale, 2, PH, PW);
  const T* fb = feat + (long)g.batch * H * W * C + cl * 8;
  for (int bin = grp; bin < PH * PW; bin += groups) {
    const int ph = bin / PW, pw = bin - ph * PW;
    BilinearTap t[4];
    uint4 v[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int iy = s >> 1, ix = s & 1;
      const float y = g.start_h + ph * g.bin_h + (iy + .5f) * g.bin_h / 2.f;
      const float x = g.start_w + pw * g.bin_w + (ix + .5f) * g.bin_w / 2.f;
      t[s] = make_tap(H, W, y, x);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      v[s][0] = *reinterpret_cast<const uint4*>(fb + ((long)t[s].y_low * W + t[s].x_low) * C);
      v[s][1] = *reinterpret_cast<const uint4*>(fb + ((long)t[s].y_low * W + t[s].x_high) * C);
      v[s][2] = *reinterpret_cast<const uint4*>(fb + ((long)t[s].y_high * W + t[s].x_low) * C);
      v[s][3] = *reinterpret_cast<const uint4*>(fb + ((long)t[s].y_high * W + t[s].x_high) * C);
    }
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float lt[8], rt[8], lb[8], rb[8];
      unpack8<T>(v[s][0], lt); unpack8<T>(v[s][1], rt); unpack8<T>(v[s][2], lb); unpack8<T>(v[s][3], rb);
      if (t[s].inside) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (t[s].w1 * lt[e] + t[s].w2 * rt[e] + t[s].w3 * lb[e] + t[s].w4 * rb[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] /= 4.f;
    T* dst = out + ((long)k * PH * PW + bin) * C + cl * 8;
    *reinterpret_cast<uint4*>(dst) = make_uint4(pack2<T>(acc[0], acc[1]), pack2<T>(acc[2], acc[3]), pack2<T>(acc[4], acc[5]), pack2<T>(acc[6], acc[7]));
  }
