// Generalized (empirical) attention core, forward only.  Replaces the energy / softmax / matmul of
// mmdet/models/plugins/generalized_attention.py:240-368 for spatial_range = -1, q_stride = 1.  The rule is stated in
// include/hvr_hip.h.  One kernel, grid (tiles of kGaQT queries, heads, frames), four waves:
//   prologue   the position terms of the workgroup's 64 queries go to LDS in f32: ex[ql][xk] = qg . Px[x][xk] + Gx[x][xk] and
//              ey[ql][yk] = qg . Py[y][yk] + Gy[y][yk], a dot product per entry (x = p % W, y = p / W PER QUERY: a tile that spans two
//              image rows needs nothing else).  They are 1 / Hk + 1 / Wk of the energies and never leave the workgroup.
//   key loop   kGaKB keys at a time: K [key][c], V TRANSPOSED [c][key] and per key (appr_bias . k, xk, yk) are staged in LDS.  A wave
//              owns 16 queries and computes the TRANSPOSED score tile S^T = K Q^T with 16x16x16 MFMAs: lane l ends with the scores of
//              keys 4 * (l / 16) + i of a 16-key tile for query l % 16, which is the B-operand layout of the second product
//              O^T = V^T P^T -- the probabilities go from registers into the MFMA, after ONE rounding into the operand type.
//              Online softmax per query: running maximum m, running sum (of the ROUNDED probabilities, so that a constant v comes back
//              as itself), accumulators rescaled by exp(m_old - m_new).  A query's 64 scores of a block sit in 4 lanes: the maximum
//              takes two xor shuffles, the sum is kept per lane and merged once at the end, in a fixed order.
//   epilogue   o = acc / sum, one rounding, 8-byte stores.
// No energy or probability tensor exists in memory, no atomics, no workspace.
#include "common.h"

namespace hvr {

constexpr int kGaQT = 64;          // queries per workgroup (16 per wave)
constexpr int kGaKB = 64;          // keys per step of the online softmax
constexpr int kGaMaxPos = 512;     // Hk + Wk the position terms of a workgroup may have (LDS)
constexpr int kGaVtPitch = kGaKB + 4;

int gen_attn_query_tile() { return kGaQT; }
int gen_attn_key_block() { return kGaKB; }

typedef short ga_s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 ga_f16x4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ f32x4 ga_mfma(const uint2& a, const uint2& b, const f32x4& c) {
  if constexpr (std::is_same<T, bf16_t>::value)
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(ga_s16x4, a), __builtin_bit_cast(ga_s16x4, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(ga_f16x4, a), __builtin_bit_cast(ga_f16x4, b), c, 0, 0, 0);
}

// sum_c a[c] * b[c] over 8 elements of the operand type, f32
template <typename T> __device__ __forceinline__ float ga_dot8(const uint4& a, const uint4& b, float acc) {
  const uint32_t ua[4] = {a.x, a.y, a.z, a.w}, ub[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a0, a1, b0, b1;
    unpack2<T>(ua[i], a0, a1);
    unpack2<T>(ub[i], b0, b1);
    acc = fmaf(a0, b0, acc);
    acc = fmaf(a1, b1, acc);
  }
  return acc;
}

struct GaArgs {
  const void *q, *k, *v;             // [B][P][heads * D], [B][Mk][heads * D] x 2; q / k may be null
  const float* ab;                   // appr_bias [heads * D] or null
  const void *px, *py;               // [heads][W][Wk][D], [heads][H][Hk][D] or null (together)
  const float *gx, *gy;              // [heads][W][Wk], [heads][H][Hk] or null (together)
  void* o;                           // [B][P][heads * D]
  int heads, H, W, Hk, Wk, qk;       // qk: the q . k term is present
};

template <typename T, int D>
__global__ __launch_bounds__(256) void gen_attn_kernel(const GaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ga_lds[];
  constexpr int KP = D + 8;                       // pitch of a staged key row (16-byte aligned rows)
  T* Ks = reinterpret_cast<T*>(ga_lds);           // [kGaKB][KP]
  T* Vt = Ks + kGaKB * KP;                        // [D][kGaVtPitch]
  float4* info = reinterpret_cast<float4*>(Vt + D * kGaVtPitch);   // [kGaKB]: (appr_bias . k or -inf past the last key, xk, yk, -)
  const int pitchx = a.Wk | 1, pitchy = a.Hk | 1; // odd: the 16 queries of a wave read 16 banks
  float* ex = reinterpret_cast<float*>(info + kGaKB);              // [kGaQT][pitchx]
  float* ey = ex + kGaQT * pitchx;                                 // [kGaQT][pitchy]

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int head = (int)blockIdx.y, b = (int)blockIdx.z;
  const int P = a.H * a.W, Mk = a.Hk * a.Wk, CQ = a.heads * D;
  const int p0 = (int)blockIdx.x * kGaQT;
  const T* qb = a.q ? reinterpret_cast<const T*>(a.q) + ((long)b * P) * CQ + head * D : nullptr;
  const T* kb = a.k ? reinterpret_cast<const T*>(a.k) + ((long)b * Mk) * CQ + head * D : nullptr;
  const T* vb = reinterpret_cast<const T*>(a.v) + ((long)b * Mk) * CQ + head * D;
  const bool pos = a.gx != nullptr || a.px != nullptr;

  // ---- prologue: the position terms of this tile's queries
  if (pos) {
    for (int axis = 0; axis < 2; ++axis) {
      const int nk = axis == 0 ? a.Wk : a.Hk, pitch = axis == 0 ? pitchx : pitchy, nq = axis == 0 ? a.W : a.H;
      const T* tab = reinterpret_cast<const T*>(axis == 0 ? a.px : a.py);
      const float* gt = axis == 0 ? a.gx : a.gy;
      float* dst = axis == 0 ? ex : ey;
      for (int idx = tid; idx < kGaQT * nk; idx += 256) {
        const int ql = idx / nk, kk = idx - ql * nk, p = p0 + ql;
        float val = 0.f;
        if (p < P) {
          const int yq = p / a.W, xq = p - yq * a.W;
          const long row = ((long)head * nq + (axis == 0 ? xq : yq)) * nk + kk;
          if (gt) val = gt[row];
          if (tab) {
            const uint4* tq = reinterpret_cast<const uint4*>(qb + (long)p * CQ);
            const uint4* tp = reinterpret_cast<const uint4*>(tab + row * D);
            float d0 = 0.f;
#pragma unroll
            for (int c = 0; c < D / 8; ++c) d0 = ga_dot8<T>(tq[c], tp[c], d0);
            val += d0;
          }
        }
        dst[ql * pitch + kk] = val;
      }
    }
  }

  // ---- this lane's query as the B operand of S^T = K Q^T: q[query c16][16 kc + 4 g .. + 3]
  const int pq = p0 + wave * 16 + c16;
  uint2 qreg[D / 16];
#pragma unroll
  for (int kc = 0; kc < D / 16; ++kc) {
    qreg[kc] = make_uint2(0, 0);
    if (a.qk && pq < P) qreg[kc] = *reinterpret_cast<const uint2*>(qb + (long)pq * CQ + kc * 16 + 4 * g);
  }
  const float* exq = ex + (wave * 16 + c16) * pitchx;
  const float* eyq = ey + (wave * 16 + c16) * pitchy;

  f32x4 acc[D / 16];
#pragma unroll
  for (int ct = 0; ct < D / 16; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;

  for (int k0 = 0; k0 < Mk; k0 += kGaKB) {
    __syncthreads();                               // the block before is read; (first pass) the prologue is written
    // stage K rows and V transposed; keys past the last are zeros (their probability is 0, and 0 * 0 adds nothing)
    for (int i = tid; i < kGaKB * (D / 8); i += 256) {
      const int key = i / (D / 8), part = i - key * (D / 8);
      const bool ok = k0 + key < Mk;
      uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (ok) {
        const long off = (long)(k0 + key) * CQ + part * 8;
        if (a.qk) kv = *reinterpret_cast<const uint4*>(kb + off);
        vv = *reinterpret_cast<const uint4*>(vb + off);
      }
      *reinterpret_cast<uint4*>(Ks + key * KP + part * 8) = kv;
      const uint32_t w4[4] = {vv.x, vv.y, vv.z, vv.w};
      unsigned short* vt = reinterpret_cast<unsigned short*>(Vt) + (part * 8) * kGaVtPitch + key;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vt[(2 * e) * kGaVtPitch] = (unsigned short)(w4[e] & 0xffffu);
        vt[(2 * e + 1) * kGaVtPitch] = (unsigned short)(w4[e] >> 16);
      }
    }
    if (tid < kGaKB) {
      const int kk = k0 + tid;
      float bk = -INFINITY;
      int xk = 0, yk = 0;
      if (kk < Mk) {
        yk = kk / a.Wk;
        xk = kk - yk * a.Wk;
        bk = 0.f;
        if (a.ab) {
          const T* kr = kb + (long)kk * CQ;
          const float* ab = a.ab + head * D;
#pragma unroll
          for (int c = 0; c < D; c += 4) {
            float kf[4];
            load4(kr + c, kf);
#pragma unroll
            for (int e = 0; e < 4; ++e) bk = fmaf(ab[c + e], kf[e], bk);
          }
        }
      }
      info[tid] = make_float4(bk, __int_as_float(xk), __int_as_float(yk), 0.f);
    }
    __syncthreads();

    // scores of this lane: keys k0 + 16 kt + 4 g + i (i = 0..3) for query c16
    f32x4 s[kGaKB / 16];
    float mn = m;
#pragma unroll
    for (int kt = 0; kt < kGaKB / 16; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a.qk) {
#pragma unroll
        for (int kc = 0; kc < D / 16; ++kc) {
          const uint2 ka = *reinterpret_cast<const uint2*>(Ks + (kt * 16 + c16) * KP + kc * 16 + 4 * g);
          s[kt] = ga_mfma<T>(ka, qreg[kc], s[kt]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 ki = info[kt * 16 + 4 * g + i];
        float e = s[kt][i] + ki.x;
        if (pos) e += exq[__float_as_int(ki.y)] + eyq[__float_as_int(ki.z)];
        s[kt][i] = e;
        mn = fmaxf(mn, e);
      }
    }
    mn = fmaxf(mn, __shfl_xor(mn, 16, 64));
    mn = fmaxf(mn, __shfl_xor(mn, 32, 64));          // finite: a block holds at least one key
    const float alpha = __expf(m - mn);              // (first block: exp(-inf) = 0 on zero accumulators)
    m = mn;
    lsum *= alpha;
#pragma unroll
    for (int ct = 0; ct < D / 16; ++ct) acc[ct] *= alpha;
#pragma unroll
    for (int kt = 0; kt < kGaKB / 16; ++kt) {
      float pr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) pr[i] = __expf(s[kt][i] - mn);
      const uint2 pb = make_uint2(pack2<T>(pr[0], pr[1]), pack2<T>(pr[2], pr[3]));
      float r0, r1, r2, r3;
      unpack2<T>(pb.x, r0, r1);
      unpack2<T>(pb.y, r2, r3);
      lsum += (r0 + r1) + (r2 + r3);
#pragma unroll
      for (int ct = 0; ct < D / 16; ++ct) {
        const uint2 va = *reinterpret_cast<const uint2*>(Vt + (ct * 16 + c16) * kGaVtPitch + kt * 16 + 4 * g);
        acc[ct] = ga_mfma<T>(va, pb, acc[ct]);
      }
    }
  }

  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (pq < P) {
    const float inv = 1.f / lsum;
    T* orow = reinterpret_cast<T*>(a.o) + ((long)b * P + pq) * CQ + head * D;
#pragma unroll
    for (int ct = 0; ct < D / 16; ++ct) {
      const float ov[4] = {acc[ct][0] * inv, acc[ct][1] * inv, acc[ct][2] * inv, acc[ct][3] * inv};
      store4(orow + ct * 16 + 4 * g, ov);
    }
  }
}

size_t gen_attn_lds_bytes(int D, int Hk, int Wk) {
  return (size_t)kGaKB * (D + 8) * 2 + (size_t)D * kGaVtPitch * 2 + (size_t)kGaKB * 16 + (size_t)kGaQT * ((Wk | 1) + (Hk | 1)) * 4;
}

int gen_attn_max_pos() { return kGaMaxPos; }

template <typename T, int D> static hipError_t launch_gen_attn(const GaArgs& a, int B, hipStream_t st) {
  static std::atomic<unsigned> attr_dev{0};   // (the attribute is per device)
  per_device_once(attr_dev, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gen_attn_kernel<T, D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)gen_attn_lds_bytes(D, kGaMaxPos, 0));
  });
  const int P = a.H * a.W;
  hipLaunchKernelGGL((gen_attn_kernel<T, D>), dim3((P + kGaQT - 1) / kGaQT, a.heads, B), dim3(256), gen_attn_lds_bytes(D, a.Hk, a.Wk), st, a);
  return hipGetLastError();
}

template <typename T> static hipError_t launch_gen_attn_d(const GaArgs& a, int B, int D, hipStream_t st) {
  if (D == 16) return launch_gen_attn<T, 16>(a, B, st);
  if (D == 32) return launch_gen_attn<T, 32>(a, B, st);
  if (D == 64) return launch_gen_attn<T, 64>(a, B, st);
  return hipErrorInvalidValue;
}

hipError_t run_gen_attn(const void* q, const void* k, const void* v, const float* ab, const void* px, const void* py, const float* gx,
                        const float* gy, void* o, int B, int heads, int D, int H, int W, int Hk, int Wk, int qk, int dtype, hipStream_t st) {
  GaArgs a;
  a.q = q; a.k = k; a.v = v; a.ab = ab; a.px = px; a.py = py; a.gx = gx; a.gy = gy; a.o = o;
  a.heads = heads; a.H = H; a.W = W; a.Hk = Hk; a.Wk = Wk; a.qk = qk;
  if (dtype == DT_BF16) return launch_gen_attn_d<bf16_t>(a, B, D, st);
  if (dtype == DT_F16) return launch_gen_attn_d<f16_t>(a, B, D, st);
  return hipErrorInvalidValue;
}

}  // namespace hvr
