// Body fragment, included INSIDE a kernel (no include guard: it is statements, not declarations): the bins of one RoI through the generic
// NHWC forward.  Features [B][H][W][C], output [K][PH][PW][C]; CV channels per lane, the workgroup's remaining lane groups spread over
// the bins.  In scope at the point of inclusion: the types / constants T, CV and
//   const T* feat; const float* roi (the RoI's five floats); T* out; int k, C, H, W, PH, PW, sample_num; float spatial_scale.
// roi_align.hip and fpn.hip include this text, so both compile the same statements (a shared inline function is not enough: the
// compiler contracts products and sums differently once the body has been a function of its own).
  const int lanes_c = C / CV;  // threads along channels
  const int groups = blockDim.x / lanes_c;
  const int cl = threadIdx.x % lanes_c, grp = threadIdx.x / lanes_c;
  if (grp >= groups) return;
  const RoiGeom g = roi_geom(roi, spatial_scale, sample_num, PH, PW);
  const T* fb = feat + (long)g.batch * H * W * C + cl * CV;
  for (int bin = grp; bin < PH * PW; bin += groups) {
    const int ph = bin / PW, pw = bin - ph * PW;
    float acc[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) acc[e] = 0.f;
    for (int iy = 0; iy < g.sn_h; ++iy) {
      const float y = g.start_h + ph * g.bin_h + (iy + .5f) * g.bin_h / (float)g.sn_h;
      for (int ix = 0; ix < g.sn_w; ++ix) {
        const float x = g.start_w + pw * g.bin_w + (ix + .5f) * g.bin_w / (float)g.sn_w;
        const BilinearTap t = make_tap(H, W, y, x);
        if (!t.inside) continue;
        float lt[CV], rt[CV], lb[CV], rb[CV];
#pragma unroll
        for (int e = 0; e < CV; e += 4) {
          load4(fb + ((long)t.y_low * W + t.x_low) * C + e, lt + e);
          load4(fb + ((long)t.y_low * W + t.x_high) * C + e, rt + e);
          load4(fb + ((long)t.y_high * W + t.x_low) * C + e, lb + e);
          load4(fb + ((long)t.y_high * W + t.x_high) * C + e, rb + e);
        }
#pragma unroll
        for (int e = 0; e < CV; ++e) acc[e] += (t.w1 * lt[e] + t.w2 * rt[e] + t.w3 * lb[e] + t.w4 * rb[e]);
      }
    }
    const float cnt = (float)(g.sn_h * g.sn_w);
#pragma unroll
    for (int e = 0; e < CV; ++e) acc[e] /= cnt;
    T* dst = out + ((long)k * PH * PW + bin) * C + cl * CV;
#pragma unroll
    for (int e = 0; e < CV; e += 4) store4(dst + e, acc + e);
  }
