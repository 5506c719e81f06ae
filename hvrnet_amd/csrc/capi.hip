// extern "C" surface of libhvr_hip.so (declarations + contracts: include/hvr_hip.h).
// Argument validation lives here; kernels assume validated inputs.
#include "../../include/hvr_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "common.h"
#include "gemm_params.h"
#include "relation_bt.h"
#include "ga_rpn.h"
#include "nms_dev.h"

namespace hvr {
hipError_t run_transpose_pad(const void*, void*, int, int, long, long, int, hipStream_t);
hipError_t run_zero_fill(void*, size_t, hipStream_t);
hipError_t run_pack_conv_weights_multi(const void*, int, long, int, hipStream_t);
hipError_t run_transpose_multi(const void*, int, int, hipStream_t);
hipError_t run_im2col_t(const void*, void*, int, int, int, int, int, int, int, int, int, int, long, hipStream_t);
hipError_t run_relu_bwd_t(const void*, const void*, void*, void*, int, int, long, hipStream_t);
hipError_t run_splitk_reduce(const float*, float*, int, int, long, int, hipStream_t);
hipError_t run_unpack_conv_wgrads_multi(const void*, int, long, int, hipStream_t);
hipError_t run_splitk_reduce_bf16(const float*, void*, int, int, long, int, hipStream_t);
hipError_t run_splitk_reduce_f16(const float*, void*, int, int, long, int, hipStream_t);
hipError_t run_splitk_reduce_half_batched(const float*, void*, int, int, long, int, int, int, long, long, hipStream_t);
hipError_t run_splitk_reduce_epi_bf16(const float*, void*, int, int, long, int, const float*, const void*, long, int, hipStream_t);
hipError_t run_relation_normalize(void*, const float*, const float*, int, int, long, int, float, hipStream_t);
hipError_t run_relu_bwd(const void*, const void*, void*, long, int, hipStream_t);
hipError_t run_im2col_nhwc(const void*, void*, int, int, int, int, int, int, int, int, int, int, int, hipStream_t);
hipError_t run_scale_rows(const void*, const float*, void*, int, long, int, hipStream_t);
hipError_t run_sgd_step(float*, const float*, float*, long, float, float, float, float, float, float*, int, hipStream_t);
hipError_t run_colsum(const void*, float*, int, int, long, int, float*, hipStream_t);
int colsum_slices(int M, int N);
size_t sgd_workspace_bytes();
hipError_t run_pack_conv_weight(const float*, const float*, void*, int, int, int, int, hipStream_t);
hipError_t run_unpack_conv_wgrad(const float*, const float*, float*, int, int, int, int, hipStream_t);
hipError_t run_det_loss(const float*, int, int, int, int, const long long*, const float*, const float*, const float*, int, float, float,
                        float, float*, float*, const int*, hipStream_t);
size_t assign_workspace_bytes(int n, int k);
hipError_t run_max_iou_assign(const float*, int, int, const float*, int, const uint8_t*, float, float, float, float, long long*, float*,
                              void*, hipStream_t);
hipError_t run_sample(const long long*, const float*, int, int, int, double, long long*, int*, hipStream_t);
hipError_t run_box_targets(const float*, int, int, const float*, const long long*, const long long*, const long long*, const int*, int,
                           const float*, const float*, float, int, long long*, float*, float*, float*, hipStream_t);
hipError_t run_rpn_loss(const float*, int, int, int, const long long*, const float*, const float*, const float*, const int*, float, float*,
                        float*, hipStream_t);
hipError_t run_ce_rows(const float*, int, int, int, const long long*, int, float*, hipStream_t);
void focal_split(int N, int C, int* S, int* rows);
hipError_t run_focal_elem(const void*, int, const long long*, const float*, int, int, float, float, int, float*, hipStream_t);
hipError_t run_focal_fused(const float*, int, const long long*, const float*, int, int, float, float, float, float, const int*, float*, float*, float*,
                           hipStream_t);
hipError_t run_rpn_focal_loss(const float*, int, int, int, const long long*, const float*, const float*, const float*, const int*, float, float, float,
                              float, float, float*, float*, hipStream_t);
hipError_t run_reg_elem(int, const float*, int, const float*, const float*, int, int, const float*, float*, hipStream_t);
hipError_t run_reg_fused(int, const float*, int, const float*, const float*, int, int, const float*, float, float, const int*, float*, float*, float*,
                         hipStream_t);
hipError_t run_box_elem(int, const float*, const float*, const float*, int, float, float, float*, hipStream_t);
hipError_t run_box_fused(int, const float*, const float*, const float*, int, float, float, float, float, const int*, float*, float*, float*, hipStream_t);
void ghm_split(int N, int C, int* S, long* per);
size_t ghm_workspace_words(int N, int C);
hipError_t run_ghmc(const float*, const float*, const long long*, const float*, int, int, int, const float*, int, float, float*, float, void*, float*,
                    float*, hipStream_t);
hipError_t run_ghmr(const float*, const float*, const float*, int, int, float, const float*, int, float, float*, float, void*, float*, float*,
                    hipStream_t);
hipError_t run_triplet_margin(const void*, long, const void*, long, int, int, int, const long long*, const long long*, const long long*, int,
                              float, int, float*, float*, float*, float*, hipStream_t);
hipError_t run_ingest(const uint8_t*, int, int, long, float*, int, int, int, int, const float*, const float*, int, int, hipStream_t);
size_t tta_merge_proposals_workspace_bytes(int A, int T, int mx);
hipError_t run_tta_merge_proposals(const float*, const int*, int, int, int, const float*, const float*, const int*, float, int, float*, int*, void*,
                                   hipStream_t);
hipError_t run_tta_map_rois(const float*, int, int, int, const float*, const float*, const int*, float*, hipStream_t);
hipError_t run_tta_merge_dets(const float*, const float*, int, int, int, const float*, const float*, const int*, float*, float*, hipStream_t);
hipError_t run_mining_argreduce(const float*, int, int, long, const long long*, const long long*, long long*, hipStream_t);
hipError_t run_relation_dscore(const void*, const void*, const void*, const void*, void*, int, long, int, long, long, float, int, hipStream_t);
hipError_t run_im2col_stem(const float*, void*, int, int, int, int, int, int, int, hipStream_t);
hipError_t run_maxpool3x3s2(const void*, void*, int, int, int, int, int, int, int, hipStream_t);
hipError_t run_cast(const void*, void*, long, int, int, float, hipStream_t);
hipError_t run_permute(const void*, void*, int, int, int, int, int, int, hipStream_t);
hipError_t run_det_decode(const float*, int, int, int, int, const float*, int, const float*, const float*, float, float,
                          float, float, float*, float*, hipStream_t);
hipError_t run_roi_align_fwd(const void*, const float*, void*, int, int, int, int, int, int, int, float, int, int, int,
                             hipStream_t);
hipError_t run_roi_align_bwd(const float*, const float*, float*, int, int, int, int, int, int, float, int, int, hipStream_t);
hipError_t run_deform_im2col(const void*, const float*, void*, int, int, int, int, int, int, int, int, int, int, int, int, long, int, int,
                             hipStream_t);
hipError_t run_deform_roi_pool(const void*, const float*, const float*, const float*, void*, int, int, int, int, int, int, int, int, int, int, int,
                               float, float, long, long, int, hipStream_t);
hipError_t run_roi_pool_fwd(const void*, const float*, void*, int32_t*, int, int, int, int, int, int, int, float, int, hipStream_t);
hipError_t run_roi_pool_bwd(const float*, const float*, const int32_t*, float*, int, int, int, int, int, int, int, hipStream_t);
hipError_t run_fpn_merge(const void* const*, void* const*, int, int, const int*, const int*, int, int, hipStream_t);
int roi_align_levels_instance(int C, int dtype);
hipError_t run_roi_align_levels(const void* const*, const int*, const int*, const float*, int, int, int, int, int, int, int, float, const float*,
                                const float*, void*, int*, hipStream_t);
hipError_t run_nms_batched(const float*, int, int, float, int, int, int, long long*, int*, const NmsWs&, hipStream_t, int band = 0,
                           int* band_done = nullptr);
hipError_t run_rpn_select(const void*, const void*, long, long, float*, const RpnParams&, int, hipStream_t);
hipError_t run_rpn_select_wide(const void*, const void*, long, long, float*, const RpnParams&, const RpnWideWs&, hipStream_t);
int rpn_wide_max_frames(int set);
hipError_t run_rpn_gather(const float*, const long long*, const int*, int, int, int, int, int, float*, int*, hipStream_t);
hipError_t run_multiclass_nms(const float*, const float*, int, int, float, float, int, float*, long long*, int*, const McNmsWs&,
                              hipStream_t);
size_t multiclass_nms_workspace_bytes(int R, int ncls);
int multiclass_nms_max_candidates();
hipError_t run_soft_nms(const float*, int, float, int, float, float, float*, long long*, int*, hipStream_t);
hipError_t run_multiclass_soft_nms(const float*, const float*, int, int, int, float, float, int, float, float, int, float*, long long*, int*,
                                   const McSoftNmsWs&, hipStream_t);
hipError_t run_seq_nms(const float*, const float*, int, const int*, int, int, int, float, float, float, int, int, float*, long long*, int*, int*,
                       int*, float*, int*, int, const SeqNmsWs&, int, hipStream_t);
hipError_t run_stem_fused(const float*, const void*, const float*, void*, int, int, int, int, hipStream_t);
hipError_t run_gconv3x3(const void*, const void*, void*, const float*, int, int, int, int, int, int, int, int, int, hipStream_t);
hipError_t run_res2_conv3x3(const void*, long, const void*, long, void*, long, const void*, const float*, int, int, int, int, int, int, int, int,
                            hipStream_t);
hipError_t run_avgpool(const void*, long, void*, long, int, int, int, int, int, int, int, int, int, int, int, hipStream_t);
hipError_t run_stem3x3s2_first(const float*, const float*, const float*, void*, int, int, int, int, int, hipStream_t);
void gcb_split(int B, int P, int* S, int* chunk);
hipError_t run_gcb_pool(const void*, const float*, float*, int, int, int, int, hipStream_t);
hipError_t run_gcb_transform(const float*, int, int, int, int, const float* const*, const float* const*, float*, float*, hipStream_t);
hipError_t run_gcb_apply(const void*, const float*, const float*, const void*, void*, int, int, int, int, int, hipStream_t);
void gn_split(int B, int P, int* S, int* chunk);
hipError_t run_gn_stats(const void*, float*, int, int, int, int, int, hipStream_t);
hipError_t run_gn_apply(const void*, const float*, const float*, const float*, float, const void*, const float*, const float*, const float*, void*, int,
                        int, int, int, int, int, hipStream_t);
int gen_attn_query_tile();
int gen_attn_key_block();
int gen_attn_max_pos();
hipError_t run_gen_attn(const void*, const void*, const void*, const float*, const void*, const void*, const float*, const float*, void*, int, int, int,
                        int, int, int, int, int, int, hipStream_t);
hipError_t run_ga_mask_offsets(const float*, long, float, unsigned char*, const float*, long, const float*, float*, long, int, long, hipStream_t);
int masked_conv_max_cout();
hipError_t run_masked_conv(const void*, const void*, const float*, const unsigned char*, float*, int, int, int, int, int, int, int, long, int,
                           hipStream_t);
hipError_t run_ga_select(const float*, const float*, const float*, const unsigned char*, float*, int*, int*, int*, const GaParams&, hipStream_t);
hipError_t run_ga_gather(const float*, const long long*, const int*, const int*, const int*, const int*, int, int, int, int, float*, int*,
                         hipStream_t);
}  // namespace hvr

using namespace hvr;

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
static int check_launch(hipError_t e, const char* what) {
  if (e == hipSuccess) return HVR_OK;
  if (e == hipErrorInvalidValue) return fail(HVR_EUNSUPPORTED, "%s: shape outside the implemented envelope", what);
  return fail(HVR_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
}
static inline int elem_size(int dtype) { return (dtype == HVR_BF16 || dtype == HVR_F16) ? 2 : 4; }   // (split half: 4 bytes per logical element)
static inline int kstep_elems(int dtype) { return (dtype == HVR_F32 || dtype == HVR_F16S) ? 32 : 64; }
static inline bool valid_dtype(int dtype) { return dtype >= HVR_F32 && dtype <= HVR_F16S; }
static inline bool aligned128(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 127) == 0; }   // a split-half [32 hi | 32 lo] group
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" {

int hvr_abi_version(void) { return 7; }  // 2: hvr_gemm_desc / hvr_conv_desc carry the few-row split-K scratch (ws, ws_bytes); 3: HVR_F16 / HVR_F16S; 4: hvr_tail_next_desc carries alpha / beta; 5: hvr_relation_fwd_grouped; 6: hvr_gemm_splitk_batched / hvr_unpack_conv_wgrads_multi; 7: hvr_sample_pos_neg takes neg_pos_ub as a double
const char* hvr_last_error(void) { return g_err.c_str(); }

static int fill_linear(GemmParams& p, const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb,
                       long ldc, int dtype, int staging) {
  std::memset(&p, 0, sizeof p);
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "dtype %d is none of HVR_F32 / HVR_BF16 / HVR_F16 / HVR_F16S", dtype);
  const int bke = kstep_elems(dtype);
  if (!A || !B || !C) return fail(HVR_EINVAL, "null operand pointer");
  if (M <= 0 || N <= 0 || K <= 0) return fail(HVR_EINVAL, "empty problem M=%d N=%d K=%d", M, N, K);
  if (K % bke) return fail(HVR_EINVAL, "K=%d is not a multiple of the %d-element K-step", K, bke);
  if (N % 4) return fail(HVR_EINVAL, "N=%d is not a multiple of 4", N);
  if (!aligned16(A) || !aligned16(B) || !aligned16(C)) return fail(HVR_EINVAL, "operands must be 16-byte aligned");
  // split half: rows are whole [64 hi | 64 lo] groups and a matrix starts on a group boundary
  if (dtype == HVR_F16S && (lda % 32 || ldb % 32 || !aligned128(A) || !aligned128(B)))
    return fail(HVR_EINVAL, "split-half operands need 128-byte aligned bases and row pitches that are multiples of 32 elements");
  // the tile loaders keep 32-bit byte offsets into A and B
  const long es = elem_size(dtype);
  if ((long)M * lda * es >= (1L << 31) || (long)N * ldb * es >= (1L << 31))
    return fail(HVR_EUNSUPPORTED, "operand of 2 GiB or more (M=%d lda=%ld N=%d ldb=%ld)", M, lda, N, ldb);
  p.A = A; p.B = B; p.C = C;
  p.M = M; p.N = N; p.K = K;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.dtype = dtype;
  p.staging = staging ? 1 : 0;
  return HVR_OK;
}

// K slices for a tile-engine product (linear layer or conv) whose 128 x 64 tile grid leaves most of the chip idle (0 / 1 = not split): the slices bring
// the launch to ~1.5 workgroups per CU, at least 4 K-steps each
static int fewrow_mode() {   // HVR_CONV_SPLITK: 0 = few-row forms off; 1 (default) = kpar.hip where it applies, else K slices + reduce; 2 = always the latter
  static const int on = std::getenv("HVR_CONV_SPLITK") ? std::atoi(std::getenv("HVR_CONV_SPLITK")) : 1;
  return on;
}
static int fewrow_slices(const GemmParams& p) {
  const int on = fewrow_mode();
  constexpr int target = 512, mink = 8, minper = 4;
  if (!on || p.dtype != DT_BF16 || !p.staging || p.out_f32 || p.tile_hint != 0) return 1;
  if (p.N % 8 || p.ldc % 8 || (p.resid && p.ldr % 8) || !aligned16(p.C) || (p.resid && !aligned16(p.resid)) || (p.bias && !aligned16(p.bias))) return 1;
  const long tiles = (long)((p.M + 127) / 128) * ((p.N + 63) / 64);
  const int ksteps = p.K / 64;
  if (tiles > 160 || ksteps < mink) return 1;
  long s = (target + tiles / 2) / tiles;
  if (s > ksteps / minper) s = ksteps / minper;
  return s < 2 ? 1 : (int)s;
}

// split-K form of a tile-engine product: f32 partial tiles [slice][M][N] from the 128 x 64 shape (three workgroups per CU),
// then one reduce + epilogue pass
static hipError_t run_fewrow_split(const GemmParams& p, int slices, void* ws, hipStream_t stream) {
  GemmParams q = p;
  const int ksteps = p.K / 64;
  q.ksplit_steps = (ksteps + slices - 1) / slices;
  q.ksplit_count = (ksteps + q.ksplit_steps - 1) / q.ksplit_steps;
  q.csplit_bytes = (long)p.M * p.N * 4;
  q.C = ws; q.ldc = p.N; q.out_f32 = 1;
  q.bias = nullptr; q.resid = nullptr; q.relu = 0;
  q.tile_hint = 2;
  hipError_t e = run_tile_op(q, EPI_LINEAR, stream);
  if (e == hipSuccess) e = run_splitk_reduce_epi_bf16((const float*)ws, p.C, p.M, p.N, p.ldc, q.ksplit_count, p.bias, p.resid, p.ldr, p.relu, stream);
  return e;
}

static int gemm_params(const hvr_gemm_desc* d, GemmParams& p) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  int rc = fill_linear(p, d->A, d->B, d->C, d->M, d->N, d->K, d->lda, d->ldb, d->ldc, d->dtype, d->staging);
  if (rc) return rc;
  const int es = elem_size(d->dtype);
  if ((d->lda * es) % 16 || (d->ldb * es) % 16) return fail(HVR_EINVAL, "lda/ldb rows must be 16-byte multiples");
  if ((d->ldc * (d->out_f32 ? 4 : es)) % 8) return fail(HVR_EINVAL, "ldc rows must be 8-byte multiples");
  if (d->dtype == HVR_F16S) {
    if (!d->out_f32 && (d->N % 8 || d->ldc % 32 || !aligned128(d->C))) return fail(HVR_EINVAL, "split-half output: N %% 8 == 0, ldc %% 32 == 0, 128-byte aligned C");
    if (d->resid && (d->N % 8 || d->ldr % 32 || !aligned128(d->resid))) return fail(HVR_EINVAL, "split-half residual: N %% 8 == 0, ldr %% 32 == 0, 128-byte aligned");
  }
  p.bias = d->bias; p.resid = d->resid; p.ldr = d->ldr; p.relu = d->relu; p.out_f32 = d->out_f32;
  p.tile_hint = d->tile_hint;
  p.alpha = d->alpha; p.beta = d->beta;
  return 0;
}

// ---- what runs for a product: ONE plan per entry, read by its launch and by every query about it ----
enum Route {
  kRouteNone = 0,    // no kernel takes the descriptor (the launch says why)
  kRoutePanel,       // row panel (expand.hip)
  kRoutePanelSplit,  // row panel on split-half operands (expand_split.hip)
  kRouteConv3x3C64,  // the 64-channel 3x3 (conv3x3.hip)
  kRouteBigTile,     // 288 x 256 tiles (bigtile.hip)
  kRouteTwoLevel,    // tile engine, two-level accumulation (EPI_LINEAR2)
  kRoutePc,          // producer / consumer tiles (pc_gemm.hip), pc_bn columns
  kRouteKpar,        // few rows: K sliced across the waves of a workgroup (kpar.hip)
  kRouteSplitK,      // few rows: `slices` K slices across workgroups + a reduce launch
  kRouteTile,        // tile engine
};
struct ProductPlan {
  GemmParams p;   // as the route's launcher takes it
  int route;
  int slices;     // > 1: the few-row rule offers the product this many K slices (taken when the caller hands the scratch for them)
  int pc_bn;
};
static size_t fewrow_bytes(const ProductPlan& r) { return r.slices > 1 ? (size_t)r.slices * r.p.M * r.p.N * 4 : 0; }
// The few-row step, the last before the tile engine: (a caller that hands a few-row workspace asked for the few-row forms: K sliced
// across the waves of a workgroup where the shape allows -- no partials, one launch -- else across workgroups + a reduce launch).
// have_ws: the size queries plan as if the scratch were there.
static void plan_fewrow(ProductPlan& r, bool have_ws, const void* ws, size_t ws_bytes) {
  r.slices = fewrow_slices(r.p);
  if (r.slices > 1 && (have_ws || (ws && aligned16(ws) && ws_bytes >= fewrow_bytes(r))))
    r.route = (fewrow_mode() == 1 && kpar_supported(r.p)) ? kRouteKpar : kRouteSplitK;
}

static int gemm_plan(const hvr_gemm_desc* d, bool have_ws, ProductPlan& r) {
  GemmParams& p = r.p;
  const int rc = gemm_params(d, p);
  if (rc) return rc;
  r.route = kRouteTile; r.slices = 1; r.pc_bn = 128;
  int hint = d->tile_hint;
  if (hint == kBigForce) {
    r.route = bigtile_supported(p, true) ? kRouteBigTile : kRouteNone;
    return 0;
  }
  if (hint == kBigHint || hint == 0) {  // the 288 x 256 shape where it applies (kBigHint: a throughput caller), else as with hint 0
    const bool thr = hint == kBigHint;
    p.tile_hint = hint = 0;
    if (bigtile_supported(p, thr)) { r.route = kRouteBigTile; return 0; }
  }
  if (d->tile_hint == kPcHint128 || d->tile_hint == kPcHint256) {
    r.pc_bn = d->tile_hint == kPcHint256 ? 256 : 128;
    r.route = pc_supported(p, EPI_LINEAR) ? kRoutePc : kRouteNone;
    return 0;
  }
  // Long-K products whose 144 x 128 tile grid is one round of the chip (fc_new_1: 4500 x 1024 x 12544 -> 256 tiles of 196
  // K-steps): the producer / consumer kernel, 1.00-1.03 PF/s against the tile engine's 0.90 (tools/pc_bench.py).  Shorter K
  // loops do not amortise its one-wave-per-SIMD compute stream's prologue; there the tile engine stays ahead.
  if (hint == 0 && d->K >= 8192 && pc_supported(p, EPI_LINEAR)) {
    const long tiles = (long)((d->M + 143) / 144) * ((d->N + 127) / 128);
    if (tiles > 192 && tiles <= 256) { r.route = kRoutePc; return 0; }
  }
  plan_fewrow(r, have_ws, d->ws, d->ws_bytes);
  return 0;
}

size_t hvr_gemm_fewrow_workspace_bytes(const hvr_gemm_desc* d) {
  ProductPlan r;
  if (gemm_plan(d, true, r)) return 0;
  // Query and launch disagree under kBigHint: the launch clears the hint before the few-row rule sees it and would take the few-row
  // forms if handed a workspace; this query has always applied the rule to the caller's hint, which refuses any hint but 0.  No
  // caller plans with it; the answer stays as it was.
  if (d->tile_hint == kBigHint) return 0;
  return fewrow_bytes(r);
}

int hvr_gemm(const hvr_gemm_desc* d, void* stream) {
  ProductPlan r;
  const int rc = gemm_plan(d, false, r);
  if (rc) return rc;
  const GemmParams& p = r.p;
  hipStream_t s = (hipStream_t)stream;
  switch (r.route) {
    case kRouteBigTile: return check_launch(run_bigtile(p, s), "hvr_gemm(big tile)");
    case kRoutePc: return check_launch(run_pc(p, EPI_LINEAR, r.pc_bn, s), "hvr_gemm (pc)");
    case kRouteKpar: return check_launch(run_kpar(p, s), "hvr_gemm(K-parallel waves)");
    case kRouteSplitK: return check_launch(run_fewrow_split(p, r.slices, d->ws, s), "hvr_gemm(split-K)");
    case kRouteTile: return check_launch(run_tile_op(p, EPI_LINEAR, s), "hvr_gemm");
    default:
      if (d->tile_hint == kBigForce) return fail(HVR_EUNSUPPORTED, "the big-tile kernel takes bf16 products with N %% 256 == 0 and K %% 64 == 0");
      return fail(HVR_EUNSUPPORTED, "the producer / consumer tile kernel takes aligned bf16 operands with N %% 8 == 0");
  }
}

// slices for a GEMM whose output has too few tiles to fill the chip and whose K loop is long (weight gradients)
static int splitk_slices(int M, int N, int K, int dtype) {
  const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
  if (dtype == HVR_F16S) return 1;   // (the three-pass K loop is not sliced)
  const int ksteps = K / kstep_elems(dtype);
  if (tiles >= 192 || ksteps < 32) return 1;
  long s = (512 + tiles - 1) / tiles;
  if (s > ksteps / 8) s = ksteps / 8;
  if (s > 64) s = 64;
  return s < 2 ? 1 : (int)s;
}

size_t hvr_gemm_splitk_workspace_bytes(int M, int N, int K, int dtype) {
  if (M <= 0 || N <= 0 || K <= 0 || !valid_dtype(dtype)) return 0;
  const int s = splitk_slices(M, N, K, dtype);
  return s > 1 ? (size_t)s * M * N * 4 : 0;
}

int hvr_gemm_splitk(const hvr_gemm_desc* d, void* ws, size_t ws_bytes, void* stream) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  if (d->bias || d->resid || d->relu) return fail(HVR_EINVAL, "split-K products have no epilogue (bias / residual / ReLU)");
  if (d->dtype != HVR_F32 && !d->out_f32) return fail(HVR_EINVAL, "split-K products are f32 (set out_f32)");
  GemmParams p;
  int rc = fill_linear(p, d->A, d->B, d->C, d->M, d->N, d->K, d->lda, d->ldb, d->ldc, d->dtype, d->staging);
  if (rc) return rc;
  const int es = elem_size(d->dtype);
  if ((d->lda * es) % 16 || (d->ldb * es) % 16) return fail(HVR_EINVAL, "lda/ldb rows must be 16-byte multiples");
  if ((d->ldc * 4) % 8) return fail(HVR_EINVAL, "ldc rows must be 8-byte multiples");
  p.out_f32 = d->out_f32;
  p.tile_hint = d->tile_hint;
  const int slices = splitk_slices(d->M, d->N, d->K, d->dtype);
  if (slices <= 1) return check_launch(run_tile_op(p, EPI_LINEAR, (hipStream_t)stream), "hvr_gemm_splitk");
  const size_t need = (size_t)slices * d->M * d->N * 4;
  if (!ws || ws_bytes < need || !aligned16(ws)) return fail(HVR_EINVAL, "split-K workspace too small (%zu < %zu) or unaligned", ws_bytes, need);
  const int ksteps = d->K / kstep_elems(d->dtype);
  p.ksplit_steps = (ksteps + slices - 1) / slices;
  p.ksplit_count = (ksteps + p.ksplit_steps - 1) / p.ksplit_steps;
  p.csplit_bytes = (long)d->M * d->N * 4;
  p.C = ws;
  p.ldc = d->N;
  hipError_t e = run_tile_op(p, EPI_LINEAR, (hipStream_t)stream);
  if (e == hipSuccess) e = run_splitk_reduce((const float*)ws, (float*)d->C, d->M, d->N, d->ldc, p.ksplit_count, (hipStream_t)stream);
  return check_launch(e, "hvr_gemm_splitk");
}

// `count` products of ONE shape in one launch (the weight gradients of a stage's identical blocks): problem g's operands sit stride_a /
// stride_b elements behind problem 0's, its f32 output stride_c floats behind; the tile engine's batch dimension (gridDim.z), K slices
// (gridDim.y) while count x tiles leaves the chip idle, and one reduce over all problems' partials
static int splitk_slices_batched(int M, int N, int K, int dtype, int count) {
  const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128) * count;
  if (dtype == HVR_F16S) return 1;
  const int ksteps = K / kstep_elems(dtype);
  if (tiles >= 384 || ksteps < 32) return 1;
  long s = (512 + tiles - 1) / tiles;
  if (s > ksteps / 8) s = ksteps / 8;
  if (s > 64) s = 64;
  return s < 2 ? 1 : (int)s;
}

size_t hvr_gemm_splitk_batched_workspace_bytes(int M, int N, int K, int dtype, int count) {
  if (M <= 0 || N <= 0 || K <= 0 || count <= 0 || !valid_dtype(dtype)) return 0;
  const int s = splitk_slices_batched(M, N, K, dtype, count);
  return s > 1 ? (size_t)s * count * M * N * 4 : 0;
}

int hvr_gemm_splitk_batched(const hvr_gemm_desc* d, int count, int64_t stride_a, int64_t stride_b, int64_t stride_c, void* ws, size_t ws_bytes,
                            void* stream) {
  if (!d || count <= 0) return fail(HVR_EINVAL, "null descriptor / count <= 0");
  if (d->bias || d->resid || d->relu) return fail(HVR_EINVAL, "split-K products have no epilogue (bias / residual / ReLU)");
  if (d->dtype != HVR_F32 && !d->out_f32) return fail(HVR_EINVAL, "split-K products are f32 (set out_f32)");
  if (d->dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "batched split-K products take f32 / bf16 / half operands");
  GemmParams p;
  int rc = fill_linear(p, d->A, d->B, d->C, d->M, d->N, d->K, d->lda, d->ldb, d->ldc, d->dtype, d->staging);
  if (rc) return rc;
  const int es = elem_size(d->dtype);
  if ((d->lda * es) % 16 || (d->ldb * es) % 16 || (stride_a * es) % 16 || (stride_b * es) % 16) return fail(HVR_EINVAL, "lda / ldb rows and the problem strides must be 16-byte multiples");
  if ((d->ldc * 4) % 8 || (stride_c * 4) % 16) return fail(HVR_EINVAL, "ldc rows must be 8-byte, stride_c 16-byte multiples");
  if (stride_a * es >= (1L << 31) || stride_b * es >= (1L << 31)) return fail(HVR_EUNSUPPORTED, "one problem's operands must stay below 2 GiB");
  p.out_f32 = d->out_f32;
  p.tile_hint = d->tile_hint;
  p.batch = count;
  p.gs_a = stride_a * es; p.gs_b = stride_b * es; p.gs_c = stride_c * 4;
  const int slices = splitk_slices_batched(d->M, d->N, d->K, d->dtype, count);
  if (slices <= 1) return check_launch(run_tile_op(p, EPI_LINEAR, (hipStream_t)stream), "hvr_gemm_splitk_batched");
  if (d->ldc != d->N || stride_c != (int64_t)d->M * d->N) return fail(HVR_EINVAL, "the sliced form writes one contiguous [count][M][N] output (ldc = N, stride_c = M * N)");
  const size_t need = (size_t)slices * count * d->M * d->N * 4;
  if (!ws || ws_bytes < need || !aligned16(ws)) return fail(HVR_EINVAL, "split-K workspace too small (%zu < %zu) or unaligned", ws_bytes, need);
  if ((long)count * d->M > 0x7fffffffL) return fail(HVR_EUNSUPPORTED, "too many output rows");
  const int ksteps = d->K / kstep_elems(d->dtype);
  p.ksplit_steps = (ksteps + slices - 1) / slices;
  p.ksplit_count = (ksteps + p.ksplit_steps - 1) / p.ksplit_steps;
  p.csplit_bytes = (long)count * d->M * d->N * 4;   // slice s of problem g: ws + s * csplit_bytes + g * M * N * 4
  p.gs_c = (long)d->M * d->N * 4;
  p.C = ws;
  p.ldc = d->N;
  hipError_t e = run_tile_op(p, EPI_LINEAR, (hipStream_t)stream);
  if (e == hipSuccess) e = run_splitk_reduce((const float*)ws, (float*)d->C, count * d->M, d->N, d->N, p.ksplit_count, (hipStream_t)stream);
  return check_launch(e, "hvr_gemm_splitk_batched");
}

static int expand_enabled() {   // HVR_EXPAND=0: the automatic choice of the row-panel kernels is off
  static const int on = std::getenv("HVR_EXPAND") ? std::atoi(std::getenv("HVR_EXPAND")) : 1;
  return on;
}

// descriptor -> kernel parameters + what runs; a negative return is the error
static int conv_plan(const hvr_conv_desc* d, bool have_ws, ProductPlan& r) {
  GemmParams& p = r.p;
  r.route = kRouteTile; r.slices = 1; r.pc_bn = 0;
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  const int OH = (d->H + 2 * d->pad - d->dil * (d->KH - 1) - 1) / d->stride + 1;
  const int OW = (d->W + 2 * d->pad - d->dil * (d->KW - 1) - 1) / d->stride + 1;
  if (OH <= 0 || OW <= 0) return fail(HVR_EINVAL, "empty conv output %dx%d", OH, OW);
  if (!valid_dtype(d->dtype)) return fail(HVR_EINVAL, "bad dtype %d", d->dtype);
  const int bke = kstep_elems(d->dtype);
  if (d->Cin % bke) return fail(HVR_EINVAL, "Cin=%d is not a multiple of %d", d->Cin, bke);
  if (d->dtype == HVR_F16S && !d->out_f32 && (d->Cout % 32 || !aligned128(d->y))) return fail(HVR_EINVAL, "split-half conv output: Cout %% 32 == 0, 128-byte aligned y");
  if (d->dtype == HVR_F16S && d->resid && (d->Cout % 32 || !aligned128(d->resid))) return fail(HVR_EINVAL, "split-half conv residual: Cout %% 32 == 0, 128-byte aligned");
  const long M = (long)d->B * OH * OW;
  if (M > 0x7fffffffL) return fail(HVR_EUNSUPPORTED, "too many output pixels");
  if ((long)d->B * d->H * d->W * d->Cin * (long)elem_size(d->dtype) >= (1L << 31))
    return fail(HVR_EUNSUPPORTED, "conv input of 2 GiB or more");
  const int K = d->KH * d->KW * d->Cin;
  int rc = fill_linear(p, d->x, d->w, d->y, (int)M, d->Cout, K, d->Cin, K, d->Cout, d->dtype, d->staging);
  if (rc) return rc;
  const bool pointwise = d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0;
  if (!pointwise) {
    if (!d->zero) return fail(HVR_EINVAL, "conv needs the zero page");
    p.conv = 1; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.OH = OH; p.OW = OW; p.KH = d->KH; p.KW = d->KW;
    p.stride = d->stride; p.pad = d->pad; p.dil = d->dil; p.zero = d->zero;
  }
  p.bias = d->bias; p.resid = d->resid; p.ldr = d->Cout; p.relu = d->relu; p.out_f32 = d->out_f32;
  p.tile_hint = d->tile_hint;
  p.alpha = d->alpha; p.beta = d->beta;
  if (pointwise) p.zero = d->zero;  // (expand.hip reads it in place of a missing shift)
  // the expand convs of a Bottleneck (1x1, K <= 256, + residual) are HBM-bound: row-panel kernel (expand.hip)
  const int use_expand = expand_enabled();
  const int hint = d->tile_hint;
  if (hint == kBigForce) {
    r.route = bigtile_supported(p, true) ? kRouteBigTile : kRouteNone;
    return 0;
  }
  const bool hint0 = p.tile_hint == 0 || p.tile_hint == kBigHint;  // (the big-tile hint leaves the dedicated kernels their shapes)
  bool big_first = false;  // the 288 x 256 tiles are ahead of the row-panel kernel from K = 256 on (layer 3's and res5's expand convs)
  if (hint0 && pointwise) {
    GemmParams q = p;
    q.tile_hint = 0;
    big_first = bigtile_supported(q, p.tile_hint == kBigHint);
    // (layer 3's expand + residual, K = 256: the big tiles are ahead on one clip -- 40 against 43 us for 15 frames -- and behind on a
    // batch of clips -- 60 frames: 178 - 198 against 155 - 167 us, profiles/r06_expand_ablation_raw.txt / r06_l3_fused.txt)
    if (big_first && p.resid && p.K == 256 && p.dtype != DT_F16S && p.M >= 65536 && expand_supported(p)) big_first = false;
  }
  const bool panel = pointwise && (expand_supported(p) || expand_split_supported(p)) &&
                     (hint == kExpandHint || (hint0 && use_expand && p.resid && p.N >= 2 * p.K && !big_first));
  if (hint == kExpandHint) p.tile_hint = 0;
  // layer 1's 3x3 (64 -> 64): persistent kernel with the weights resident in the LDS (conv3x3.hip)
  static const int use_c3 = std::getenv("HVR_CONV3") ? std::atoi(std::getenv("HVR_CONV3")) : 1;
  if (panel || (hint0 && use_c3 && conv3x3_c64_supported(p))) {
    r.route = !panel ? kRouteConv3x3C64 : p.dtype == DT_F16S ? kRoutePanelSplit : kRoutePanel;
    if (hint == kBigHint) p.tile_hint = 0;
    return 0;
  }
  if (hint == kTwoLevelHint) {
    // two-level accumulation (gemm_params.h: EPI_LINEAR2) where the format carries the f32 tolerance; any other format runs as with hint 0
    p.tile_hint = 0;
    if (two_level_supported(p)) { r.route = kRouteTwoLevel; return 0; }
  }
  if (hint == kBigHint || hint == 0 || hint == kTwoLevelHint) {
    p.tile_hint = 0;
    if (bigtile_supported(p, hint == kBigHint)) { r.route = kRouteBigTile; return 0; }
  }
  plan_fewrow(r, have_ws, d->ws, d->ws_bytes);
  return 0;
}

// Where query and launch disagree (no caller plans with these hints -- ResNet.stage_route uses 0 and kBigHint; the answers stay as
// they were):
//  - hvr_conv2d_path has always answered 0 under kBigForce and kTwoLevelHint, where the launch runs the big tiles (kBigForce: or
//    fails) or, under kTwoLevelHint, the two-level form, else the big tiles where they apply;
//  - hvr_conv2d_splitk_workspace_bytes has always applied the few-row rule to the caller's hint, which refuses kBigHint and
//    kTwoLevelHint; the launch clears those hints first and would take the few-row forms if handed a workspace.
int hvr_conv2d_path(const hvr_conv_desc* d) {
  ProductPlan r;
  const int rc = conv_plan(d, false, r);
  if (rc) return rc;
  if (d->tile_hint == kBigForce || d->tile_hint == kTwoLevelHint) return 0;
  switch (r.route) {
    case kRoutePanel: case kRoutePanelSplit: return 1;
    case kRouteConv3x3C64: return 2;
    case kRouteBigTile: return 3;
    default: return 0;
  }
}

size_t hvr_conv2d_splitk_workspace_bytes(const hvr_conv_desc* d) {
  ProductPlan r;
  if (conv_plan(d, true, r)) return 0;
  if (d->tile_hint == kBigHint || d->tile_hint == kTwoLevelHint) return 0;
  return fewrow_bytes(r);
}

int hvr_conv2d_nhwc(const hvr_conv_desc* d, void* stream) {
  ProductPlan r;
  const int rc = conv_plan(d, false, r);
  if (rc) return rc;
  const GemmParams& p = r.p;
  hipStream_t s = (hipStream_t)stream;
  switch (r.route) {
    case kRoutePanel: return check_launch(run_expand(p, s), "hvr_conv2d_nhwc(expand)");
    case kRoutePanelSplit: return check_launch(run_expand_split(p, s), "hvr_conv2d_nhwc(expand)");
    case kRouteConv3x3C64: return check_launch(run_conv3x3_c64(p, s), "hvr_conv2d_nhwc(conv3x3_c64)");
    case kRouteBigTile: return check_launch(run_bigtile(p, s), "hvr_conv2d_nhwc(big tile)");
    case kRouteTwoLevel: return check_launch(run_tile_op(p, EPI_LINEAR2, s), "hvr_conv2d_nhwc(two-level)");
    case kRouteKpar: return check_launch(run_kpar(p, s), "hvr_conv2d_nhwc(K-parallel waves)");
    case kRouteSplitK: return check_launch(run_fewrow_split(p, r.slices, d->ws, s), "hvr_conv2d_nhwc(split-K)");
    case kRouteTile: return check_launch(run_tile_op(p, EPI_LINEAR, s), "hvr_conv2d_nhwc");
    default: return fail(HVR_EUNSUPPORTED, "the big-tile kernel takes bf16 convs with Cout %% 256 == 0 and Cin %% 64 == 0");
  }
}

static int tail_params(const hvr_tail_desc* d, GemmParams& p) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  if (d->dtype != HVR_BF16 && d->dtype != HVR_F16) return fail(HVR_EUNSUPPORTED, "hvr_bottleneck_tail takes bf16 or half operands");
  if (d->B <= 0 || d->OH <= 0 || d->OW <= 0 || d->stride2 <= 0) return fail(HVR_EINVAL, "empty tail problem");
  if ((d->OH - 1) * d->stride2 >= d->H2 || (d->OW - 1) * d->stride2 >= d->W2) return fail(HVR_EINVAL, "the sampled pixels fall outside x");
  const long M = (long)d->B * d->OH * d->OW;
  if (M > 0x7fffffffL) return fail(HVR_EUNSUPPORTED, "too many output pixels");
  const int K = d->C1 + d->C2;
  int rc = fill_linear(p, d->h, d->w, d->y, (int)M, d->Cout, K, d->C1, K, d->Cout, d->dtype, 1);
  if (rc) return rc;
  if (!d->x || !aligned16(d->x)) return fail(HVR_EINVAL, "x must be a 16-byte aligned device pointer");
  if ((long)d->B * d->H2 * d->W2 * d->C2 * 2 >= (1L << 31)) return fail(HVR_EUNSUPPORTED, "block input of 2 GiB or more");
  p.bias = d->bias; p.relu = d->relu;
  p.A2 = d->x; p.K1 = d->C1; p.H2 = d->H2; p.W2 = d->W2; p.s2 = d->stride2; p.OH = d->OH; p.OW = d->OW;
  return 0;
}

// the tile engine's form of the fused tail (K too long for the row-panel kernel: stage 3's 256 + 512 and res5's 512 + 1024):
// one GEMM over K = C1 + C2 whose A operand switches from h to the sampled block input at K-step C1 / 64
static bool tail_on_tile_engine(const GemmParams& p) {
  return (p.dtype == DT_BF16 || p.dtype == DT_F16) && p.K1 % 64 == 0 && (p.K - p.K1) % 64 == 0 && p.K1 >= 64 && p.K - p.K1 >= 64 && p.N % 8 == 0 && p.ldc % 8 == 0 &&
         (long)p.M * (p.K - p.K1) * 2 < (1L << 31);
}

static int tail_route(const GemmParams& p) {
  if (expand_supported(p)) return kRoutePanel;
  if (!tail_on_tile_engine(p)) return kRouteNone;
  // the 288 x 256 tiles take the second K segment too (same MFMA order: bit-identical).  Round 3 measured them slightly behind the tile
  // engine here; with persistent workgroups (round 6) they are ahead: res5's 512 + 1024 -> 2048 tail 973 -> 857 us for four clips (230 ->
  // 200 for one), layer 3's 256 + 512 -> 1024 311 -> 256 (72 -> 69)
  return bigtile_supported(p, false) ? kRouteBigTile : kRouteTile;
}

int hvr_bottleneck_tail_supported(const hvr_tail_desc* d) {
  GemmParams p;
  return !tail_params(d, p) && tail_route(p) != kRouteNone;
}

int hvr_bottleneck_tail(const hvr_tail_desc* d, void* stream) {
  GemmParams p;
  const int rc = tail_params(d, p);
  if (rc) return rc;
  switch (tail_route(p)) {
    case kRoutePanel: return check_launch(run_expand(p, (hipStream_t)stream), "hvr_bottleneck_tail");
    case kRouteBigTile: return check_launch(run_bigtile(p, (hipStream_t)stream), "hvr_bottleneck_tail(big tile)");
    case kRouteTile: return check_launch(run_tile_op(p, EPI_LINEAR, (hipStream_t)stream), "hvr_bottleneck_tail(tile engine)");
    default: return fail(HVR_EUNSUPPORTED, "no fused tail kernel for C1=%d C2=%d Cout=%d", d->C1, d->C2, d->Cout);
  }
}

// closing 1x1 (+ projection shortcut or identity residual) + the next block's reducing 1x1 (expand.hip, NX > 0)
static int tail_next_params(const hvr_tail_next_desc* d, GemmParams& p) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  const hvr_tail_desc& t = d->tail;
  if (t.C2 > 0) {
    const int rc = tail_params(&t, p);
    if (rc) return rc;
  } else {
    if (t.dtype != HVR_BF16 && t.dtype != HVR_F16 && t.dtype != HVR_F16S)
      return fail(HVR_EUNSUPPORTED, "hvr_bottleneck_tail_next takes bf16, half or (identity form) split-half operands");
    if (t.B <= 0 || t.OH <= 0 || t.OW <= 0) return fail(HVR_EINVAL, "empty tail problem");
    const long M = (long)t.B * t.OH * t.OW;
    if (M > 0x7fffffffL) return fail(HVR_EUNSUPPORTED, "too many output pixels");
    const int rc = fill_linear(p, t.h, t.w, t.y, (int)M, t.Cout, t.C1, t.C1, t.C1, t.Cout, t.dtype, 1);
    if (rc) return rc;
    const bool split = t.dtype == HVR_F16S;
    if (!d->resid || !(split ? aligned128(d->resid) : aligned16(d->resid)))
      return fail(HVR_EINVAL, "an identity block needs its (16-byte aligned; split half: 128-byte aligned) residual map");
    if (split && (t.Cout % 32 || !aligned128(t.y))) return fail(HVR_EINVAL, "split-half tail: Cout %% 32 == 0, 128-byte aligned y");
    p.bias = t.bias; p.relu = t.relu; p.resid = d->resid; p.ldr = t.Cout;
    if (t.dtype == HVR_F16S) { p.alpha = d->alpha; p.beta = d->beta; }   // (documented as split-half only: include/hvr_hip.h)
  }
  if (!t.relu) return fail(HVR_EUNSUPPORTED, "the next block reads the activated output (relu = 1)");
  p.Wn = d->wn; p.bias_n = d->bias_n; p.Hn = d->hn; p.Cn = d->Cn;
  return 0;
}

static int tail_next_route(const GemmParams& p) {
  return expand_split_next_supported(p) ? kRoutePanelSplit : expand_next_supported(p) ? kRoutePanel : kRouteNone;
}

int hvr_bottleneck_tail_next_supported(const hvr_tail_next_desc* d) {
  GemmParams p;
  return !tail_next_params(d, p) && tail_next_route(p) != kRouteNone;
}

int hvr_bottleneck_tail_next(const hvr_tail_next_desc* d, void* stream) {
  GemmParams p;
  const int rc = tail_next_params(d, p);
  if (rc) return rc;
  switch (tail_next_route(p)) {
    case kRoutePanelSplit: return check_launch(run_expand_split(p, (hipStream_t)stream), "hvr_bottleneck_tail_next(split half)");
    case kRoutePanel: return check_launch(run_expand(p, (hipStream_t)stream), "hvr_bottleneck_tail_next");
    default: return fail(HVR_EUNSUPPORTED, "no fused tail + next conv kernel for C1=%d C2=%d Cout=%d Cn=%d", d->tail.C1, d->tail.C2, d->tail.Cout, d->Cn);
  }
}

// the identity form with only the pixels (s oy, s ox) of y written, as a compact map (expand.hip / expand_split.hip, LIVE)
static int tail_next_live_params(const hvr_tail_next_live_desc* d, GemmParams& p) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  const hvr_tail_desc& t = d->next.tail;
  if (t.C2 != 0) return fail(HVR_EUNSUPPORTED, "hvr_bottleneck_tail_next_live is the identity form (tail.C2 == 0)");
  if (d->live_stride <= 0) return fail(HVR_EINVAL, "live_stride must be positive");
  const int rc = tail_next_params(&d->next, p);
  if (rc) return rc;
  p.live = d->live_stride; p.OH = t.OH; p.OW = t.OW;
  return 0;
}

static int tail_next_live_route(const GemmParams& p) {
  return expand_split_next_live_supported(p) ? kRoutePanelSplit : expand_next_live_supported(p) ? kRoutePanel : kRouteNone;
}

int hvr_bottleneck_tail_next_live_supported(const hvr_tail_next_live_desc* d) {
  GemmParams p;
  return !tail_next_live_params(d, p) && tail_next_live_route(p) != kRouteNone;
}

int hvr_bottleneck_tail_next_live(const hvr_tail_next_live_desc* d, void* stream) {
  GemmParams p;
  const int rc = tail_next_live_params(d, p);
  if (rc) return rc;
  switch (tail_next_live_route(p)) {
    case kRoutePanelSplit: return check_launch(run_expand_split(p, (hipStream_t)stream), "hvr_bottleneck_tail_next_live(split half)");
    case kRoutePanel: return check_launch(run_expand(p, (hipStream_t)stream), "hvr_bottleneck_tail_next_live");
    default:
      return fail(HVR_EUNSUPPORTED, "no live-store tail + next conv kernel for C1=%d Cout=%d Cn=%d dtype=%d", d->next.tail.C1, d->next.tail.Cout, d->next.Cn, d->next.tail.dtype);
  }
}

// closing 1x1 of a stage's last block on the pixels the next stage's stride-2 1x1 convs read: compact h and y, the residual sampled from the
// block's full-resolution input (expand.hip / expand_split.hip, GemmParams::rs)
static int close_sampled_params(const hvr_close_sampled_desc* d, GemmParams& p) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  if (!valid_dtype(d->dtype)) return fail(HVR_EINVAL, "bad dtype %d", d->dtype);
  if (d->B <= 0 || d->OH <= 0 || d->OW <= 0 || d->rstride <= 0 || d->RH <= 0 || d->RW <= 0) return fail(HVR_EINVAL, "empty sampled-close problem");
  if ((long)(d->OH - 1) * d->rstride >= d->RH || (long)(d->OW - 1) * d->rstride >= d->RW) return fail(HVR_EINVAL, "the sampled pixels fall outside resid");
  const long M = (long)d->B * d->OH * d->OW;
  if (M > 0x7fffffffL || (long)d->B * d->RH * d->RW > 0x7fffffffL) return fail(HVR_EUNSUPPORTED, "too many pixels");
  const int rc = fill_linear(p, d->h, d->w, d->y, (int)M, d->Cout, d->C1, d->C1, d->C1, d->Cout, d->dtype, 1);
  if (rc) return rc;
  const bool split = d->dtype == HVR_F16S;
  if (!d->resid || !(split ? aligned128(d->resid) : aligned16(d->resid)))
    return fail(HVR_EINVAL, "resid must be a 16-byte aligned (split half: 128-byte aligned) device pointer");
  if (split && (d->Cout % 32 || !aligned128(d->y))) return fail(HVR_EINVAL, "split-half sampled close: Cout %% 32 == 0, 128-byte aligned y");
  p.bias = d->bias; p.relu = d->relu; p.resid = d->resid; p.ldr = d->Cout;
  p.rs = d->rstride; p.RH = d->RH; p.RW = d->RW; p.OH = d->OH; p.OW = d->OW;
  if (split) { p.alpha = d->alpha; p.beta = d->beta; }
  return 0;
}

// the row-panel kernels only, and only where hvr_conv2d_nhwc takes them for the same product at full resolution (same sums, bit for bit)
static int close_sampled_route(const GemmParams& p) {
  if (!expand_enabled() || p.N < 2 * p.K) return kRouteNone;
  return expand_split_supported(p) ? kRoutePanelSplit : expand_supported(p) ? kRoutePanel : kRouteNone;
}

int hvr_bottleneck_close_sampled_supported(const hvr_close_sampled_desc* d) {
  GemmParams p;
  return !close_sampled_params(d, p) && close_sampled_route(p) != kRouteNone;
}

int hvr_bottleneck_close_sampled(const hvr_close_sampled_desc* d, void* stream) {
  GemmParams p;
  const int rc = close_sampled_params(d, p);
  if (rc) return rc;
  switch (close_sampled_route(p)) {
    case kRoutePanelSplit: return check_launch(run_expand_split(p, (hipStream_t)stream), "hvr_bottleneck_close_sampled(split half)");
    case kRoutePanel: return check_launch(run_expand(p, (hipStream_t)stream), "hvr_bottleneck_close_sampled");
    default: return fail(HVR_EUNSUPPORTED, "no sampled-residual closing kernel for C1=%d Cout=%d dtype=%d (%d output pixels)", d->C1, d->Cout, d->dtype, p.M);
  }
}

// the instance set of gconv3x3.hip (include/hvr_hip.h states it); 0 or the error
static int gconv_check(const hvr_gconv_desc* d) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  if (!valid_dtype(d->dtype)) return fail(HVR_EINVAL, "bad dtype %d", d->dtype);
  if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(HVR_EINVAL, "empty grouped conv input %dx%dx%d", d->B, d->H, d->W);
  if (d->C <= 0 || d->C % 64 || d->C > 2048) return fail(HVR_EINVAL, "grouped conv: C=%d is not a multiple of 64 in [64, 2048]", d->C);
  if (d->groups <= 0 || d->C % d->groups) return fail(HVR_EINVAL, "grouped conv: groups=%d does not divide C=%d", d->groups, d->C);
  const int Cg = d->C / d->groups;
  if (Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32) return fail(HVR_EINVAL, "grouped conv: C / groups = %d is none of 4 / 8 / 16 / 32", Cg);
  if (d->stride != 1 && d->stride != 2) return fail(HVR_EINVAL, "grouped conv: stride %d is neither 1 nor 2", d->stride);
  if (d->pad != d->dil || (d->dil != 1 && d->dil != 2)) return fail(HVR_EINVAL, "grouped conv: pad=%d dil=%d (pad == dil in {1, 2})", d->pad, d->dil);
  if (!d->x || !d->w || !d->y || !d->bias) return fail(HVR_EINVAL, "grouped conv: null operand pointer (the bias is required)");
  if (!aligned16(d->x) || !aligned16(d->w) || !aligned16(d->y) || !aligned16(d->bias)) return fail(HVR_EINVAL, "grouped conv: operands must be 16-byte aligned");
  if ((long)d->B * ((d->H - 1) / d->stride + 1) * ((d->W - 1) / d->stride + 1) > 0x7fffffffL) return fail(HVR_EINVAL, "grouped conv: too many output pixels");
  if (d->dtype != HVR_BF16 && d->dtype != HVR_F16)
    return fail(HVR_EUNSUPPORTED, "grouped conv: bf16 and half operands only (f32 / split half: hvr_conv2d_nhwc on the block-diagonal dense weight)");
  return HVR_OK;
}

int hvr_conv3x3_grouped_supported(const hvr_gconv_desc* d) { return gconv_check(d) == HVR_OK ? 1 : 0; }

int hvr_conv3x3_grouped(const hvr_gconv_desc* d, void* stream) {
  const int rc = gconv_check(d);
  if (rc) return rc;
  return check_launch(run_gconv3x3(d->x, d->w, d->y, d->bias, d->B, d->H, d->W, d->C, d->C / d->groups, d->stride, d->dil, d->relu, d->dtype,
                                   (hipStream_t)stream), "hvr_conv3x3_grouped");
}

// byte range [lo, hi) of a pitched slice: npix pixels at pitch ld elements, C channels from element off on
static inline void slice_range(const void* base, long ld, long off, long npix, int C, int es, uintptr_t& lo, uintptr_t& hi) {
  lo = reinterpret_cast<uintptr_t>(base) + (uintptr_t)off * es;
  hi = lo + (uintptr_t)((npix - 1) * ld + C) * es;
}
// 1 when a slice written at (y, ldy, y_off) may share an element with one read at (x, ldx, x_off): the address ranges overlap and the
// two are not channel-disjoint slices of maps at one pitch
static int slices_alias(const void* y, long ldy, long y_off, long ny, const void* x, long ldx, long x_off, long nx, int C, int es) {
  uintptr_t ylo, yhi, xlo, xhi;
  slice_range(y, ldy, y_off, ny, C, es, ylo, yhi);
  slice_range(x, ldx, x_off, nx, C, es, xlo, xhi);
  if (yhi <= xlo || xhi <= ylo) return 0;
  if (ldx != ldy) return 1;
  const uintptr_t pitch = (uintptr_t)ldy * es;
  const uintptr_t d = ylo >= xlo ? (ylo - xlo) % pitch : (pitch - (xlo - ylo) % pitch) % pitch;   // y's first channel inside x's pixel
  return !(d >= (uintptr_t)C * es && d + (uintptr_t)C * es <= pitch);
}

// the instance set of res2.hip's slice conv (include/hvr_hip.h states it); 0 or the error
static int res2_check(const hvr_res2_conv_desc* d) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  if (!valid_dtype(d->dtype)) return fail(HVR_EINVAL, "bad dtype %d", d->dtype);
  if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(HVR_EINVAL, "empty slice conv input %dx%dx%d", d->B, d->H, d->W);
  if (d->Wp != 32 && d->Wp != 64 && d->Wp != 128 && d->Wp != 224) return fail(HVR_EINVAL, "slice conv: Wp=%d is none of 32 / 64 / 128 / 224", d->Wp);
  if (d->stride != 1 && d->stride != 2) return fail(HVR_EINVAL, "slice conv: stride %d is neither 1 nor 2", d->stride);
  if (d->pad != d->dil || (d->dil != 1 && d->dil != 2)) return fail(HVR_EINVAL, "slice conv: pad=%d dil=%d (pad == dil in {1, 2})", d->pad, d->dil);
  if (!d->x || !d->w || !d->y || !d->bias) return fail(HVR_EINVAL, "slice conv: null operand pointer (the bias is required)");
  if (!aligned16(d->x) || !aligned16(d->w) || !aligned16(d->y) || !aligned16(d->bias) || (d->add && !aligned16(d->add)))
    return fail(HVR_EINVAL, "slice conv: operands must be 16-byte aligned");
  if (d->ldx <= 0 || d->ldx % 32 || d->x_off < 0 || d->x_off % 32 || d->x_off + d->Wp > d->ldx)
    return fail(HVR_EINVAL, "slice conv: x pitch %ld / offset %ld (multiples of 32, offset + Wp <= pitch)", (long)d->ldx, (long)d->x_off);
  if (d->ldy <= 0 || d->ldy % 32 || d->y_off < 0 || d->y_off % 32 || d->y_off + d->Wp > d->ldy)
    return fail(HVR_EINVAL, "slice conv: y pitch %ld / offset %ld (multiples of 32, offset + Wp <= pitch)", (long)d->ldy, (long)d->y_off);
  if (d->add && (d->lda <= 0 || d->lda % 32 || d->add_off < 0 || d->add_off % 32 || d->add_off + d->Wp > d->lda))
    return fail(HVR_EINVAL, "slice conv: add pitch %ld / offset %ld (multiples of 32, offset + Wp <= pitch)", (long)d->lda, (long)d->add_off);
  const long nx = (long)d->B * d->H * d->W, ny = (long)d->B * ((d->H - 1) / d->stride + 1) * ((d->W - 1) / d->stride + 1);
  if (ny > 0x7fffffffL) return fail(HVR_EINVAL, "slice conv: too many output pixels");
  if (slices_alias(d->y, d->ldy, d->y_off, ny, d->x, d->ldx, d->x_off, nx, d->Wp, 2))
    return fail(HVR_EINVAL, "slice conv: y aliases x (the output slice shares elements with the input slice)");
  if (d->add && slices_alias(d->y, d->ldy, d->y_off, ny, d->add, d->lda, d->add_off, nx, d->Wp, 2))
    return fail(HVR_EINVAL, "slice conv: y aliases add (the output slice shares elements with the added slice)");
  if (d->dtype != HVR_BF16 && d->dtype != HVR_F16)
    return fail(HVR_EUNSUPPORTED, "slice conv: bf16 and half operands only (f32 / split half: hvr_conv2d_nhwc on a contiguous copy of the slice)");
  return HVR_OK;
}

int hvr_res2_conv3x3_supported(const hvr_res2_conv_desc* d) { return res2_check(d) == HVR_OK ? 1 : 0; }

int hvr_res2_conv3x3(const hvr_res2_conv_desc* d, void* stream) {
  const int rc = res2_check(d);
  if (rc) return rc;
  const char* x = static_cast<const char*>(d->x) + d->x_off * 2;
  const char* a = d->add ? static_cast<const char*>(d->add) + d->add_off * 2 : nullptr;
  char* y = static_cast<char*>(d->y) + d->y_off * 2;
  return check_launch(run_res2_conv3x3(x, d->ldx, a, d->lda, y, d->ldy, d->w, d->bias, d->B, d->H, d->W, d->Wp, d->stride, d->dil, d->relu, d->dtype,
                                       (hipStream_t)stream), "hvr_res2_conv3x3");
}

int hvr_avgpool_nhwc(const hvr_pool_desc* d, void* stream) {
  if (!d) return fail(HVR_EINVAL, "null descriptor");
  if (!valid_dtype(d->dtype)) return fail(HVR_EINVAL, "bad dtype %d", d->dtype);
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return fail(HVR_EINVAL, "empty pool input %dx%dx%dx%d", d->B, d->H, d->W, d->C);
  if (d->k < 1 || d->k > 3) return fail(HVR_EINVAL, "avgpool: k=%d is none of 1 / 2 / 3", d->k);
  if (d->stride != 1 && d->stride != 2) return fail(HVR_EINVAL, "avgpool: stride %d is neither 1 nor 2", d->stride);
  if (d->pad < 0 || d->pad > d->k / 2) return fail(HVR_EINVAL, "avgpool: pad=%d (at most k / 2 = %d)", d->pad, d->k / 2);
  if (d->H + 2 * d->pad < d->k || d->W + 2 * d->pad < d->k) return fail(HVR_EINVAL, "avgpool: the %dx%d map is smaller than the window", d->H, d->W);
  if (d->C % 4 || d->ldx <= 0 || d->ldx % 4 || d->x_off < 0 || d->x_off % 4 || d->x_off + d->C > d->ldx || d->ldy <= 0 || d->ldy % 4 || d->y_off < 0 ||
      d->y_off % 4 || d->y_off + d->C > d->ldy)
    return fail(HVR_EINVAL, "avgpool: C=%d, pitches %ld / %ld, offsets %ld / %ld (multiples of 4, offset + C <= pitch)", d->C, (long)d->ldx, (long)d->ldy,
                (long)d->x_off, (long)d->y_off);
  if (!d->x || !d->y || !aligned16(d->x) || !aligned16(d->y)) return fail(HVR_EINVAL, "avgpool: x and y must be 16-byte aligned device pointers");
  if (d->dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "avgpool: no split-half instance (pool the f32 form)");
  int O[2];
  const int I[2] = {d->H, d->W};
  for (int i = 0; i < 2; ++i) {
    const int span = I[i] + 2 * d->pad - d->k;
    O[i] = (d->ceil_mode ? (span + d->stride - 1) / d->stride : span / d->stride) + 1;
    if (d->ceil_mode && (O[i] - 1) * d->stride >= I[i] + d->pad) --O[i];   // the last window starts inside the map or its left padding
  }
  const int es = elem_size(d->dtype);
  const long nx = (long)d->B * d->H * d->W, ny = (long)d->B * O[0] * O[1];
  if (ny * (d->C / 4) > 0x7fffffffL * 256) return fail(HVR_EINVAL, "avgpool: too many output elements");
  uintptr_t xlo, xhi, ylo, yhi;
  slice_range(d->x, d->ldx, d->x_off, nx, d->C, es, xlo, xhi);
  slice_range(d->y, d->ldy, d->y_off, ny, d->C, es, ylo, yhi);
  if (!(yhi <= xlo || xhi <= ylo)) return fail(HVR_EINVAL, "avgpool: y aliases x");
  return check_launch(run_avgpool(static_cast<const char*>(d->x) + d->x_off * es, d->ldx, static_cast<char*>(d->y) + d->y_off * es, d->ldy, d->B, d->H,
                                  d->W, O[0], O[1], d->C, d->k, d->stride, d->pad, d->count_include_pad ? 1 : 0, d->dtype, (hipStream_t)stream),
                      "hvr_avgpool_nhwc");
}

// ---- global context block (gcb.hip)
static int gcb_shape(const char* what, int B, int P, int C) {
  if (B <= 0 || P <= 0 || C <= 0) return fail(HVR_EINVAL, "%s: empty map B=%d P=%d C=%d", what, B, P, C);
  if (C % 64 || C > 2048) return fail(HVR_EUNSUPPORTED, "%s: C=%d is no multiple of 64 up to 2048", what, C);
  if ((long)B * P > 0x7fffffffL / 4) return fail(HVR_EUNSUPPORTED, "%s: %ld pixels", what, (long)B * P);
  return HVR_OK;
}
int hvr_gcb_supported(int C, int dtype) { return C > 0 && C % 64 == 0 && C <= 2048 && (dtype == HVR_F32 || dtype == HVR_BF16 || dtype == HVR_F16); }
int hvr_gcb_splits(int B, int P, int C) {
  if (B <= 0 || P <= 0 || C <= 0) return 0;
  int S, chunk;
  gcb_split(B, P, &S, &chunk);
  return S;
}
size_t hvr_gcb_workspace_bytes(int B, int P, int C) {
  const int S = hvr_gcb_splits(B, P, C);
  return align256((size_t)B * S * (C + 4) * sizeof(float));
}
int hvr_gcb_pool(const void* u, const float* wm, void* ws, size_t ws_bytes, int B, int P, int C, int dtype, void* stream) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "hvr_gcb_pool: bad dtype %d", dtype);
  if (dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "hvr_gcb_pool: no split-half instance (pool the f32 form)");
  if (int rc = gcb_shape("hvr_gcb_pool", B, P, C)) return rc;
  if (!u || !ws || !aligned16(u) || !aligned16(ws) || (wm && !aligned16(wm))) return fail(HVR_EINVAL, "hvr_gcb_pool: u, wm and ws must be 16-byte aligned device pointers");
  if (ws_bytes < hvr_gcb_workspace_bytes(B, P, C)) return fail(HVR_EWORKSPACE, "hvr_gcb_pool: workspace of %zu bytes, %zu needed", ws_bytes, hvr_gcb_workspace_bytes(B, P, C));
  return check_launch(run_gcb_pool(u, wm, (float*)ws, B, P, C, dtype, (hipStream_t)stream), "hvr_gcb_pool");
}
int hvr_gcb_transform(const void* ws, size_t ws_bytes, int B, int P, int C, int R, const hvr_gcb_mlp* mul, const hvr_gcb_mlp* add, float* m, float* t,
                      void* stream) {
  if (int rc = gcb_shape("hvr_gcb_transform", B, P, C)) return rc;
  if (R < 1 || R > 2048) return fail(R < 1 ? HVR_EINVAL : HVR_EUNSUPPORTED, "hvr_gcb_transform: %d bottleneck channels (1 .. 2048)", R);
  if (!mul && !add) return fail(HVR_EINVAL, "hvr_gcb_transform: neither fusion branch given");
  if (!ws || !aligned16(ws) || (mul && !m) || (add && !t)) return fail(HVR_EINVAL, "hvr_gcb_transform: null or misaligned pointer");
  const size_t slab_bytes = (size_t)B * hvr_gcb_splits(B, P, C) * (C + 4) * sizeof(float);   // (the partials themselves: hvr_gcb_workspace_bytes rounds up)
  if (ws_bytes < slab_bytes) return fail(HVR_EWORKSPACE, "hvr_gcb_transform: partials of %zu bytes, %zu needed", ws_bytes, slab_bytes);
  const float* pm[6];
  const float* pa[6];
  for (int k = 0; k < 2; ++k) {
    const hvr_gcb_mlp* w = k == 0 ? mul : add;
    if (!w) continue;
    const float** dst = k == 0 ? pm : pa;
    dst[0] = w->w1; dst[1] = w->b1; dst[2] = w->gamma; dst[3] = w->beta; dst[4] = w->w2t; dst[5] = w->b2;
    for (int i = 0; i < 6; ++i)
      if (!dst[i]) return fail(HVR_EINVAL, "hvr_gcb_transform: null weight pointer");
    if (!aligned16(w->w1)) return fail(HVR_EINVAL, "hvr_gcb_transform: w1 must be 16-byte aligned");
  }
  return check_launch(run_gcb_transform((const float*)ws, B, P, C, R, mul ? pm : nullptr, add ? pa : nullptr, m, t, (hipStream_t)stream), "hvr_gcb_transform");
}
int hvr_gcb_apply(const void* u, const float* m, const float* t, const void* resid, void* y, int B, int P, int C, int relu, int dtype, void* stream) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "hvr_gcb_apply: bad dtype %d", dtype);
  if (dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "hvr_gcb_apply: no split-half instance (apply on the f32 form)");
  if (int rc = gcb_shape("hvr_gcb_apply", B, P, C)) return rc;
  if (!u || !y || !aligned16(u) || !aligned16(y) || (resid && !aligned16(resid)) || (m && !aligned16(m)) || (t && !aligned16(t)))
    return fail(HVR_EINVAL, "hvr_gcb_apply: operands must be 16-byte aligned device pointers");
  // y may BE u or resid (same address); any other overlap would let one lane read what another has written
  const size_t bytes = (size_t)B * P * C * elem_size(dtype);
  const void* ins[2] = {u, resid};
  for (const void* x : ins) {
    if (!x || x == y) continue;
    const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(y);
    if (a < b + bytes && b < a + bytes) return fail(HVR_EINVAL, "hvr_gcb_apply: y overlaps an input without being it");
  }
  return check_launch(run_gcb_apply(u, m, t, resid, y, B, P, C, relu ? 1 : 0, dtype, (hipStream_t)stream), "hvr_gcb_apply");
}

// ---- group normalisation (gn.hip)
static bool gn_instance(int C, int G) {
  if (C < 64 || C > 2048 || C % 64 || G < 1 || C % G) return false;
  const int cg = C / G;
  return cg == 2 || cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64;
}
static int gn_shape(const char* what, int B, int P, int C, int G, int dtype) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "%s: bad dtype %d", what, dtype);
  if (dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "%s: no split-half instance (normalise the f32 form)", what);
  if (B <= 0 || P <= 0 || C <= 0 || G <= 0) return fail(HVR_EINVAL, "%s: empty map B=%d P=%d C=%d G=%d", what, B, P, C, G);
  if (C % 64 || C > 2048) return fail(HVR_EUNSUPPORTED, "%s: C=%d is no multiple of 64 from 64 to 2048", what, C);
  if (C % G) return fail(HVR_EUNSUPPORTED, "%s: G=%d does not divide C=%d", what, G, C);
  if (!gn_instance(C, G)) return fail(HVR_EUNSUPPORTED, "%s: Cg=%d channels per group (C=%d, G=%d) is not one of 2, 4, 8, 16, 32, 64", what, C / G, C, G);
  if (B > 65535) return fail(HVR_EUNSUPPORTED, "%s: B=%d frames (up to 65535)", what, B);
  if ((long)P * (C / G) > (1L << 24)) return fail(HVR_EUNSUPPORTED, "%s: %ld values per group and frame (up to 2^24: the counts are f32)", what, (long)P * (C / G));
  return HVR_OK;
}
int hvr_gn_supported(int C, int G, int dtype) { return gn_instance(C, G) && (dtype == HVR_F32 || dtype == HVR_BF16 || dtype == HVR_F16); }
int hvr_gn_splits(int B, int P, int C) {
  if (B <= 0 || P <= 0 || C <= 0) return 0;
  int S, chunk;
  gn_split(B, P, &S, &chunk);
  return S;
}
size_t hvr_gn_workspace_bytes(int B, int P, int C, int G) {
  if (G <= 0) return 0;
  return align256((size_t)B * hvr_gn_splits(B, P, C) * G * 4 * sizeof(float));
}
int hvr_gn_stats(const void* u, void* ws, size_t ws_bytes, int B, int P, int C, int G, int dtype, void* stream) {
  if (int rc = gn_shape("hvr_gn_stats", B, P, C, G, dtype)) return rc;
  if (!u || !ws || !aligned16(u) || !aligned16(ws)) return fail(HVR_EINVAL, "hvr_gn_stats: u and ws must be 16-byte aligned device pointers");
  if (ws_bytes < hvr_gn_workspace_bytes(B, P, C, G))
    return fail(HVR_EWORKSPACE, "hvr_gn_stats: workspace of %zu bytes, %zu needed", ws_bytes, hvr_gn_workspace_bytes(B, P, C, G));
  return check_launch(run_gn_stats(u, (float*)ws, B, P, C, G, dtype, (hipStream_t)stream), "hvr_gn_stats");
}
int hvr_gn_apply(const void* u, const void* ws, const float* gamma, const float* beta, float eps, const void* resid, const void* ws_r,
                 const float* gamma_r, const float* beta_r, void* y, int B, int P, int C, int G, int relu, int dtype, void* stream) {
  if (int rc = gn_shape("hvr_gn_apply", B, P, C, G, dtype)) return rc;
  if (!(eps > 0.f)) return fail(HVR_EINVAL, "hvr_gn_apply: eps=%g must be positive", (double)eps);
  if (!u || !y || !ws || !gamma || !beta || !aligned16(u) || !aligned16(y) || !aligned16(ws) || (resid && !aligned16(resid)) || (ws_r && !aligned16(ws_r)))
    return fail(HVR_EINVAL, "hvr_gn_apply: u, ws, resid, ws_r and y must be 16-byte aligned device pointers, gamma and beta given");
  if ((ws_r != nullptr) != (gamma_r != nullptr) || (ws_r != nullptr) != (beta_r != nullptr) || (ws_r && !resid))
    return fail(HVR_EINVAL, "hvr_gn_apply: a normalised residual takes resid, ws_r, gamma_r and beta_r together");
  // y may BE u or resid (same address); any other overlap would let one lane read what another has written
  const size_t bytes = (size_t)B * P * C * elem_size(dtype);
  const void* ins[2] = {u, resid};
  for (const void* x : ins) {
    if (!x || x == y) continue;
    const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(y);
    if (a < b + bytes && b < a + bytes) return fail(HVR_EINVAL, "hvr_gn_apply: y overlaps an input without being it");
  }
  return check_launch(run_gn_apply(u, (const float*)ws, gamma, beta, eps, resid, (const float*)ws_r, gamma_r, beta_r, y, B, P, C, G, relu ? 1 : 0, dtype,
                                   (hipStream_t)stream),
                      "hvr_gn_apply");
}

// ---- generalized attention core (gen_attn.hip)
int hvr_gen_attn_supported(int d, int heads, int Hk, int Wk, int dtype) {
  return (d == 16 || d == 32 || d == 64) && heads >= 1 && Hk >= 1 && Wk >= 1 && (long)Hk + Wk <= gen_attn_max_pos() && (dtype == HVR_BF16 || dtype == HVR_F16);
}
int hvr_gen_attn_query_tile(void) { return gen_attn_query_tile(); }
int hvr_gen_attn_key_block(void) { return gen_attn_key_block(); }
int hvr_gen_attn_fwd(const hvr_gen_attn_desc* d, void* stream) {
  if (!d) return fail(HVR_EINVAL, "hvr_gen_attn_fwd: null descriptor");
  if (d->B <= 0 || d->heads <= 0 || d->H <= 0 || d->W <= 0 || d->Hk <= 0 || d->Wk <= 0 || d->d <= 0)
    return fail(HVR_EINVAL, "hvr_gen_attn_fwd: empty problem B=%d heads=%d d=%d H=%d W=%d Hk=%d Wk=%d", d->B, d->heads, d->d, d->H, d->W, d->Hk, d->Wk);
  if (!hvr_gen_attn_supported(d->d, d->heads, d->Hk, d->Wk, d->dtype))
    return fail(HVR_EUNSUPPORTED, "hvr_gen_attn_fwd: d=%d (16 / 32 / 64), Hk + Wk = %d (<= %d), dtype %d (bf16 / half)", d->d, d->Hk + d->Wk, gen_attn_max_pos(), d->dtype);
  if ((long)d->heads * d->d > 65536 || (long)d->H * d->W > 0x7fffffffL / 4 || (long)d->Hk * d->Wk > 0x7fffffffL / 4 || d->heads > 65535 || d->B > 65535)
    return fail(HVR_EUNSUPPORTED, "hvr_gen_attn_fwd: problem too large");
  if (!d->v || !d->o) return fail(HVR_EINVAL, "hvr_gen_attn_fwd: v and o are required");
  if (!d->q != !(d->qk || d->px)) return fail(HVR_EINVAL, "hvr_gen_attn_fwd: q is given exactly when the q.k term or the q.P terms are");
  if (!d->k != !(d->qk || d->appr_bias)) return fail(HVR_EINVAL, "hvr_gen_attn_fwd: k is given exactly when the q.k term or appr_bias is");
  if (!d->px != !d->py || !d->gx != !d->gy) return fail(HVR_EINVAL, "hvr_gen_attn_fwd: the x and y tables come in pairs");
  if (!d->k && !d->gx && !d->px) return fail(HVR_EINVAL, "hvr_gen_attn_fwd: no energy term given");
  const void* ptrs[9] = {d->q, d->k, d->v, d->appr_bias, d->px, d->py, d->gx, d->gy, d->o};
  for (const void* p : ptrs)
    if (p && !aligned16(p)) return fail(HVR_EINVAL, "hvr_gen_attn_fwd: operands must be 16-byte aligned device pointers");
  return check_launch(run_gen_attn(d->q, d->k, d->v, d->appr_bias, d->px, d->py, d->gx, d->gy, d->o, d->B, d->heads, d->d, d->H, d->W, d->Hk, d->Wk,
                                   d->qk ? 1 : 0, d->dtype, (hipStream_t)stream), "hvr_gen_attn_fwd");
}

int hvr_stem3x3s2_first(const float* img, const float* w, const float* bias, void* y, int B, int H, int W, int ldy, int dtype, void* stream) {
  if (!img || !w || !bias || !y || !aligned16(img) || !aligned16(w) || !aligned16(bias) || !aligned16(y))
    return fail(HVR_EINVAL, "stem3x3s2_first: operands must be 16-byte aligned device pointers");
  if (B <= 0 || H <= 0 || W <= 0) return fail(HVR_EINVAL, "empty image %dx%dx%d", B, H, W);
  if (ldy < 32 || ldy % 4) return fail(HVR_EINVAL, "stem3x3s2_first: ldy=%d (a multiple of 4, at least 32)", ldy);
  if (dtype != HVR_F32 && dtype != HVR_BF16 && dtype != HVR_F16)
    return fail(HVR_EUNSUPPORTED, "stem3x3s2_first: f32, bf16 or half output (split half: cast the f32 output)");
  if ((long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) > 0x7fffffffL) return fail(HVR_EINVAL, "stem3x3s2_first: too many output pixels");
  return check_launch(run_stem3x3s2_first(img, w, bias, y, B, H, W, ldy, dtype, (hipStream_t)stream), "hvr_stem3x3s2_first");
}

int hvr_im2col_stem(const float* img, void* cols, int B, int H, int W, int KP, int dtype, void* stream) {
  if (!img || !cols || B <= 0) return fail(HVR_EINVAL, "bad stem arguments");
  if (dtype == HVR_F16S && (KP % 32 || !aligned128(cols))) return fail(HVR_EINVAL, "split-half patch rows: KP %% 32 == 0, 128-byte aligned");
  if (KP < 147 || KP % kstep_elems(dtype)) return fail(HVR_EINVAL, "KP=%d must be >= 147 and a K-step multiple", KP);
  const int OH = (H + 6 - 7) / 2 + 1, OW = (W + 6 - 7) / 2 + 1;
  return check_launch(run_im2col_stem(img, cols, B, H, W, OH, OW, KP, dtype, (hipStream_t)stream), "hvr_im2col_stem");
}

int hvr_stem_fused_dtype(const float* img, const void* wpk, const float* bias, void* out, int B, int H, int W, int dtype, void* stream) {
  if (!img || !wpk || !bias || !out || B <= 0 || H < 7 || W < 7) return fail(HVR_EINVAL, "bad fused-stem arguments");
  if (dtype != HVR_BF16 && dtype != HVR_F16 && dtype != HVR_F16S) return fail(HVR_EUNSUPPORTED, "the fused stem computes on bf16, half or split-half operands");
  if (!aligned16(wpk) || !aligned16(out) || !aligned16(bias)) return fail(HVR_EINVAL, "fused stem operands must be 16-byte aligned");
  if (dtype == HVR_F16S && !aligned128(out)) return fail(HVR_EINVAL, "split-half stem output must be 128-byte aligned");
  return check_launch(run_stem_fused(img, wpk, bias, out, B, H, W, dtype, (hipStream_t)stream), "hvr_stem_fused");
}
int hvr_stem_fused(const float* img, const void* wpk, const float* bias, void* out, int B, int H, int W, void* stream) {
  return hvr_stem_fused_dtype(img, wpk, bias, out, B, H, W, HVR_BF16, stream);
}

int hvr_maxpool3x3s2_nhwc(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {
  if (!x || !y || C % 4) return fail(HVR_EINVAL, "bad maxpool arguments (C %% 4 == 0 required)");
  if (dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "max pooling runs on f32 / bf16 / half maps");
  const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
  return check_launch(run_maxpool3x3s2(x, y, B, H, W, C, OH, OW, dtype, (hipStream_t)stream), "hvr_maxpool3x3s2_nhwc");
}

// ---- relation ----
static int env_tile(const char* name) {  // tuning override, read once
  const char* v = std::getenv(name);
  return v ? std::atoi(v) : 0;
}
static inline long rel_ldp(int Mk) { return ((long)Mk + 127) / 128 * 128; }

// Key-slices of the apply pass when there are few query rows (the key-frame-only stage: Mq = 300 against Mk = 4 500 gives a
// 3 x 8 output tile grid with a 72-step K loop -- 24 workgroups on 256 CUs): the 128-key blocks are dealt to `slices` workgroups
// per output tile (at least 2 blocks each), every slice writes an f32 partial, one reduce launch sums and rounds them.  The
// block weights g = 2^(m_t - m*) / L are global per row, so the partials simply add.  1 = no split.
static int apply_slice_blocks() { return 4; }   // 128-key blocks per slice of a sliced apply pass
static int apply_slices(int Mq, int Mk, int D) {
  const long tiles = (long)((Mq + 127) / 128) * ((D + 127) / 128);
  const int nblk = (int)(rel_ldp(Mk) / 128);
  if (tiles >= 96 || nblk < 8 || D % 8) return 1;
  // a FIXED four blocks (512 keys) per slice: the partition -- and with it the order of the f32 sum -- depends on Mk only,
  // so AMONG the calls that take this path (fewer than 96 output tiles: up to 1 536 query rows at D = 1024) a query row's result
  // does not depend on how many other rows are in the call.  Whether the path is taken does depend on Mq: the same row computed
  // in a 4 500-row call (unsplit, one running f32 sum over the 36 blocks) may differ from it in the last f32 bit.  The loops that
  // are tested for batch invariance (cached / look-ahead stream) always call the stages with the shapes that ship -- 300 and
  // 4 500 rows -- so each stage stays on one side of the threshold
  const int per = apply_slice_blocks();
  return (nblk + per - 1) / per;
}

// The apply pass of ONE problem on two-byte / f32 operands: O = sum_t g_t (P~_t V_t) from the scores pass's P~ and block statistics
// (the tile engine's / pc_gemm.hip's EPI_APPLY, key slices for few query rows).  Shared by hvr_relation_fwd and the per-group leg of
// hvr_relation_fwd_grouped.
static int relation_apply_pass(const void* P, const void* Vt, float* mstat, float* lstat, float* partial, void* O, int64_t ldo,
                               int Mq, int Mk, int D, long ldp, int nt, int dtype, int staging, hipStream_t s) {
  const bool two_byte = dtype == HVR_BF16 || dtype == HVR_F16;
  constexpr int tile_apply = 0, gm_apply = 1;
#ifdef HVR_DEBUG_KNOBS
  static const int dbg_ld0 = env_tile("HVR_DBG_LD0");
#endif
  GemmParams p;
  int rc;
  rc = fill_linear(p, P, Vt, O, Mq, D, (int)ldp, ldp, ldp, ldo, dtype, staging);
  if (rc) return rc;
  p.mstat = mstat; p.lstat = lstat; p.ntile = nt;
  p.tile_hint = tile_apply;
  p.group_m = gm_apply;
#ifdef HVR_DEBUG_KNOBS
  if (dbg_ld0 & 2) { p.lda = 0; p.ldb = 0; }
#endif
  const int slices = apply_slices(Mq, Mk, D);
  if (slices > 1 && tile_apply == 0 && (!two_byte || (ldo % 8 == 0 && aligned16(O)))) {
    const int steps_per_blk = two_byte ? 2 : 4;
    const int per = apply_slice_blocks();  // apply_slices: 128-key blocks per slice
    p.ksplit_steps = per * steps_per_blk;
    p.ksplit_count = slices;
    p.csplit_bytes = (long)Mq * D * 4;
    p.C = partial; p.ldc = D; p.out_f32 = two_byte ? 1 : 0;
    p.tile_hint = 1;  // 128 x 128 tiles; the slices are latency chains of 8 K-steps (the pipelined shapes measure the same)
    // (an in-launch merge of the partials by the slice that reaches an output tile last -- tickets, agent-scope fences -- was built in
    // round 3 and measured SLOWER than the 5 us reduce launch it saved: 49.3 -> 83.6 us for the stage, 27.6 us of it fences
    // (profiles/r03_key_stage_merge_ab.txt); removed in round 5)
    hipError_t e = run_tile_op(p, EPI_APPLY, s);
    if (e == hipSuccess)
      e = dtype == HVR_BF16 ? run_splitk_reduce_bf16(partial, O, Mq, D, ldo, slices, s)
          : dtype == HVR_F16 ? run_splitk_reduce_f16(partial, O, Mq, D, ldo, slices, s) : run_splitk_reduce(partial, (float*)O, Mq, D, ldo, slices, s);
    return check_launch(e, "relation: apply (key slices)");
  }
  // The producer / consumer form of the apply pass (pc_gemm.hip, 144 x 128 tiles, block weights from an LDS table).  Round 2 measured
  // it behind the tile engine (60 against 57 us) and left it opt-in; on round 4's boxes it is AHEAD, alone (tools/rel_bench.py: 0.1073 /
  // 0.1102 ms per relation call against 0.1164 / 0.1200) and inside the window (three alternating runs of tools/window_breakdown.py:
  // 109.4 / 110.3 / 110.5 us per call against 114.1 / 113.0 / 113.1) -- profiles/r04_relation_apply.txt -- so it is the default for
  // window-sized problems.
  if (Mq >= 1024 && pc_supported(p, EPI_APPLY))
    return check_launch(run_pc(p, EPI_APPLY, 128, s), "relation: apply (pc)");
  return check_launch(run_tile_op(p, EPI_APPLY, s), "relation: apply");
}

// relation_normalize_kernel / relation_normalize_split_kernel keep one factor per 128-key block of a row in a fixed LDS table
// (misc.hip, `g[128]`): the sweeps take at most kNormalizeMaxBlocks blocks = 16 384 keys.  Checked before anything is launched.
constexpr int kNormalizeMaxBlocks = 128;
static int normalize_blocks_ok(int Mk, const char* what) {
  if (rel_ldp(Mk) / 128 > kNormalizeMaxBlocks)
    return fail(HVR_EUNSUPPORTED, "%s: Mk=%d exceeds the %d keys (%d blocks of 128) the normalising sweep supports", what, Mk,
                kNormalizeMaxBlocks * 128, kNormalizeMaxBlocks);
  return HVR_OK;
}
// whether relation_split_tail normalises P~ in a sweep of its own (HVR_SPLIT_NORMALIZE = 0 / 1 forces the folded / the swept form)
static bool split_normalizes(int Mq) {
  static const int split_normalize = std::getenv("HVR_SPLIT_NORMALIZE") ? std::atoi(std::getenv("HVR_SPLIT_NORMALIZE")) : -1;
  return split_normalize == 1 || (split_normalize < 0 && Mq >= 1024);
}

// What follows the scores pass of ONE split-half problem: V^T (V == nullptr: the scores launch wrote it), then either one normalising sweep over P~ + a plain product, or the apply
// pass with the block weights g = 2^(m_t - m*) / L folded in per 128-key block (EPI_APPLY: a block is four split K-steps of three
// MFMAs, its un-scaled partial joins the running total by one FMA per accumulator register).  Shared by hvr_relation_fwd and the
// per-group leg of hvr_relation_fwd_grouped.
static int relation_split_tail(void* P, void* Vt, float* mstat, float* lstat, const void* V, int64_t ldv, void* O, int64_t ldo, int Mq,
                               int Mk, int D, long ldp, int nt, int staging, hipStream_t s) {
  constexpr int tile_apply_s = 0;
  int rc = V ? check_launch(run_transpose_pad(V, Vt, Mk, D, ldv, ldp, HVR_F16S, s), "relation: V transpose (split half)") : HVR_OK;
  if (rc) return rc;
  GemmParams p;
  rc = fill_linear(p, P, Vt, O, Mq, D, (int)ldp, ldp, ldp, ldo, HVR_F16S, staging);
  if (rc) return rc;
  p.alpha = 1.f / kSplitProbScale;   // the probabilities are stored x 2^12 (gemm_tile.h / relation_bt.hip, scores epilogue)
  p.mstat = mstat; p.lstat = lstat; p.ntile = nt;
  p.tile_hint = tile_apply_s;
#ifdef HVR_DEBUG_KNOBS
  static const int dbg_apply_s = env_tile("HVR_DBG_APPLY_S");
  if (dbg_apply_s) p.tile_hint = dbg_apply_s;
#endif
  // Which form: measured on one MI355X (tools/rel_bench.py --dtype f16x2; profiles/r04_split_relation.txt): the folded form wins
  // the key stage (300 x 4 500: 0.146 against 0.163 ms), the full stage goes the other way (4 500 x 4 500: 0.32-0.36 against
  // 0.29 ms) -- the fold needs the double-buffered apply shapes (the pipelined loop is written for two K-steps per block), and one
  // normalising sweep over P~ (22 us at 7.5 TB/s out of the Infinity Cache) + the pipelined plain product is cheaper than they are.
  // HVR_SPLIT_NORMALIZE = 0 / 1 forces the folded / the swept form.
  if (split_normalizes(Mq)) {
    rc = check_launch(run_relation_normalize(P, mstat, lstat, Mq, nt, ldp, HVR_F16S, 1.f, s), "relation: normalise (split half)");
    if (rc) return rc;
    return check_launch(run_tile_op(p, EPI_LINEAR, s), "relation: apply (split half, plain product)");
  }
  return check_launch(run_tile_op(p, EPI_APPLY, s), "relation: apply (split half)");
}

// P~ [Mq][ldp], V^T [D][ldp], the block maxima and sums [Mq][ntile] and, with apply_slices(...) > 1, the slices' f32 partial outputs [slices][Mq][D]
struct RelationWs { void *P, *Vt; float *mstat, *lstat, *partial; size_t bytes; };
static RelationWs relation_ws(void* base, int Mq, int Mk, int D, int dtype) {
  const long ldp = rel_ldp(Mk), nt = ldp / 128;
  const size_t es = elem_size(dtype);
  const int slices = apply_slices(Mq, Mk, D);
  Carver c(base);
  RelationWs L;
  L.P = c.take<char>((size_t)Mq * ldp * es);
  L.Vt = c.take<char>((size_t)D * ldp * es);
  L.mstat = c.take<float>((size_t)Mq * nt);
  L.lstat = c.take<float>((size_t)Mq * nt);
  L.partial = c.take<float>(slices > 1 ? (size_t)slices * Mq * D : 0);
  L.bytes = c.off;
  return L;
}

size_t hvr_relation_workspace_bytes(int Mq, int Mk, int D, int dtype) { return relation_ws(nullptr, Mq, Mk, D, dtype).bytes; }

// one group's score tiles on the persistent big-tile kernel (relation_bt.hip); `groups` > 1: group g's operands gs_* elements behind
// group 0's, its workspace `per` bytes behind
static ScoresBTParams scores_bt_params(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, const RelationWs& w, int Mq,
                                       int Mk, int D, float scale, int dtype, int groups = 1, int64_t gsq = 0, int64_t gsk = 0, int64_t gsv = 0,
                                       size_t per = 0, int int_max = 0) {
  const long ldp = rel_ldp(Mk);
  const long es = elem_size(dtype);
  ScoresBTParams b;
  b.Q = (const bf16_t*)Q; b.K = (const bf16_t*)K; b.P = (bf16_t*)w.P; b.mstat = w.mstat; b.lstat = w.lstat;
  b.V = (const bf16_t*)V; b.Vt = (bf16_t*)w.Vt; b.Mq = Mq; b.Mk = Mk; b.D = D; b.ntile = (int)(ldp / 128);
  b.ldq = ldq; b.ldk = ldk; b.ldv = ldv; b.ldp = ldp; b.sl2 = scale * 1.4426950408889634f;
  b.f16 = dtype == HVR_F16S ? 2 : dtype == HVR_F16;
  b.groups = groups; b.gs_q = gsq; b.gs_k = gsk; b.gs_v = gsv;
  b.gs_p = b.gs_vt = (long)(per / es); b.gs_stat = (long)(per / 4);
  b.int_max = int_max;
  return b;
}

int hvr_relation_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O,
                     int64_t ldo, int Mq, int Mk, int D, float scale, int dtype, int staging, void* ws, size_t ws_bytes,
                     void* stream) {
  if (!Q || !K || !V || !O || !ws) return fail(HVR_EINVAL, "null pointer");
  if (Mq <= 0 || Mk <= 0) return fail(HVR_EINVAL, "empty relation Mq=%d Mk=%d", Mq, Mk);
  if (!(scale > 0.f)) return fail(HVR_EINVAL, "relation scale must be positive (the reference uses 1/sqrt(D)), got %g", (double)scale);
  if (ws_bytes < hvr_relation_workspace_bytes(Mq, Mk, D, dtype))
    return fail(HVR_EWORKSPACE, "relation workspace %zu < %zu", ws_bytes, hvr_relation_workspace_bytes(Mq, Mk, D, dtype));
  const long ldp = rel_ldp(Mk);
  const int nt = (int)(ldp / 128);
  const RelationWs L = relation_ws(ws, Mq, Mk, D, dtype);
  void *P = L.P, *Vt = L.Vt;
  float *mstat = L.mstat, *lstat = L.lstat, *partial = L.partial;
  hipStream_t s = (hipStream_t)stream;

  GemmParams p;
  int rc;
  constexpr int tile_scores_s = 0;
  if (dtype == HVR_F16S) {
    // split half: the scores pass (block-local maxima, P~ stored x 2^12 in the split format) -- on the 352 x 256 persistent tiles of
    // relation_bt.hip for window-sized problems, else on the tile engine -- then relation_split_tail
    if (ldv % 64 || !aligned128(V) || ldo % 32 || !aligned128(O) || D % 64) return fail(HVR_EINVAL, "split-half relation: D, ldv multiples of 64, ldo of 32, 128-byte aligned V / O");
    if (split_normalizes(Mq) && (rc = normalize_blocks_ok(Mk, "split-half relation"))) return rc;
    const bool bt = staging && scores_bt_supported(Mq, Mk, D, ldq, ldk, ldv, ldp, Q, K, V, P, Vt, 1, true);
    if (bt) {   // (V^T is written by the same launch)
      rc = check_launch(run_scores_bt(scores_bt_params(Q, ldq, K, ldk, V, ldv, L, Mq, Mk, D, scale, dtype), s), "relation: scores (split half, big tile)");
    } else {
      rc = fill_linear(p, Q, K, P, Mq, (Mk + 3) / 4 * 4, D, ldq, ldk, ldp, dtype, staging);
      if (rc) return rc;
      p.N = Mk; p.scale = scale; p.mstat = mstat; p.lstat = lstat; p.ntile = nt; p.group_m = 8;
      p.tile_hint = tile_scores_s;
      rc = check_launch(run_tile_op(p, EPI_SCORES, s), "relation: scores (split half)");
    }
    if (rc) return rc;
    return relation_split_tail(P, Vt, mstat, lstat, bt ? nullptr : V, ldv, O, ldo, Mq, Mk, D, ldp, nt, staging, s);
  }
  const bool two_byte = dtype == HVR_BF16 || dtype == HVR_F16;
  // tuning overrides, read once
  constexpr int tile_scores = 0, gm_scores = 8;
#ifdef HVR_DEBUG_KNOBS  // tuning builds only (tools/build_var.sh NAME "-DHVR_DEBUG_KNOBS ..." capi ...): alias every operand row to row 0 (no memory-system cost)
  static const int dbg_ld0 = env_tile("HVR_DBG_LD0");
#endif
  const bool bt = two_byte && staging && scores_bt_supported(Mq, Mk, D, ldq, ldk, ldv, ldp, Q, K, V, P, Vt);
  if (bt) {
    // window-sized problems: one 336 x 256 score tile per CU, V^T written by the same launch (relation_bt.hip)
    rc = check_launch(run_scores_bt(scores_bt_params(Q, ldq, K, ldk, V, ldv, L, Mq, Mk, D, scale, dtype), s), "relation: scores (big tile)");
    if (rc) return rc;
  } else {
    // few query rows (the key stage, 300 x 4 500: 108 score tiles on 256 CUs): V^T is written by workgroups of the SCORES launch that sit
    // behind its tiles, on the CUs the score grid leaves idle -- one launch and ~8 us less than the transpose launch in front of it
    // (GemmParams::tr_*, gemm_tile.h)
    const bool fold = two_byte && staging && Mq <= 1024 && D % 8 == 0 && ldv % 8 == 0 && aligned16(V) && aligned16(Vt);
    if (!fold) {
      rc = check_launch(run_transpose_pad(V, Vt, Mk, D, ldv, ldp, dtype, s), "relation: V transpose");
      if (rc) return rc;
    }
    rc = fill_linear(p, Q, K, P, Mq, (Mk + 3) / 4 * 4, D, ldq, ldk, ldp, dtype, staging);
    if (rc) return rc;
    if (fold) {
      p.tr_in = V; p.tr_out = Vt; p.tr_R = Mk; p.tr_C = D; p.tr_ldx = ldv; p.tr_ldt = ldp;
      const int score_tiles = ((Mq + 127) / 128) * ((Mk + 127) / 128);   // (the 128 x 128 shape below)
      const int vt_tiles = ((D + 63) / 64) * (int)((ldp + 63) / 64);
      int nb = 256 - score_tiles % 256;   // one workgroup per CU the last round of score tiles leaves free
      if (nb < 64) nb += 256;
      p.tr_blocks = nb < vt_tiles ? nb : vt_tiles;
    }
    p.N = Mk;  // keys beyond Mk are masked inside the score epilogue
    p.scale = scale; p.mstat = mstat; p.lstat = lstat; p.ntile = nt;
    // (few query rows -- the key stage, 300 x 4 500: 108 tiles walking 16 K-steps each -- are a latency chain: the 4-stage ring
    // of the 128 x 128 shape keeps three K-steps of DMA in flight, 54.3 -> 50.8 us for the stage)
    p.tile_hint = tile_scores ? tile_scores : ((two_byte && staging && Mq <= 1024) ? 9 : 0);
    p.group_m = gm_scores;
#ifdef HVR_DEBUG_KNOBS
    if (dbg_ld0 & 1) { p.lda = 0; p.ldb = 0; }
#endif
    rc = check_launch(run_tile_op(p, EPI_SCORES, s), "relation: scores");
    if (rc) return rc;
  }
  return relation_apply_pass(P, Vt, mstat, lstat, partial, O, ldo, Mq, Mk, D, ldp, nt, dtype, staging, s);
}

// ---- relation, G independent problems of one shape in one call (the windows a caller has in flight) ----
size_t hvr_relation_grouped_workspace_bytes(int groups, int Mq, int Mk, int D, int dtype) {
  return (size_t)(groups > 0 ? groups : 0) * align256(hvr_relation_workspace_bytes(Mq, Mk, D, dtype));
}

int hvr_relation_fwd_grouped(const void* Q, int64_t ldq, int64_t gsq, const void* K, int64_t ldk, int64_t gsk, const void* V, int64_t ldv,
                             int64_t gsv, void* O, int64_t ldo, int64_t gso, int groups, int Mq, int Mk, int D, float scale, int dtype,
                             int staging, int exact, void* ws, size_t ws_bytes, void* stream) {
  if (!Q || !K || !V || !O || !ws) return fail(HVR_EINVAL, "null pointer");
  if (groups <= 0) return fail(HVR_EINVAL, "relation groups must be positive, got %d", groups);
  if (Mq <= 0 || Mk <= 0) return fail(HVR_EINVAL, "empty relation Mq=%d Mk=%d", Mq, Mk);
  if (!(scale > 0.f)) return fail(HVR_EINVAL, "relation scale must be positive (the reference uses 1/sqrt(D)), got %g", (double)scale);
  if (gsq < 0 || gsk < 0 || gsv < 0 || gso < 0) return fail(HVR_EINVAL, "negative group stride");
  const size_t per = align256(hvr_relation_workspace_bytes(Mq, Mk, D, dtype));
  if (ws_bytes < per * (size_t)groups) return fail(HVR_EWORKSPACE, "grouped relation workspace %zu < %zu", ws_bytes, per * (size_t)groups);
  const size_t es = elem_size(dtype);
  hipStream_t s = (hipStream_t)stream;
  // HVR_REL_GROUPED (tuning): 0 = one hvr_relation_fwd per group; 1 = the persistent scores launch over all groups, apply per group;
  // 2 (default) = + the 288 x 256 apply launch over all groups where it applies (bf16, >= 3 window-sized groups)
  static const int mode = std::getenv("HVR_REL_GROUPED") ? std::atoi(std::getenv("HVR_REL_GROUPED")) : 2;
  const long ldp = rel_ldp(Mk);
  const int nt = (int)(ldp / 128);
  const bool two_byte = dtype == HVR_BF16 || dtype == HVR_F16;
  // group 0's workspace laid out as hvr_relation_fwd lays out its own; group g's `per` bytes further
  const RelationWs L = relation_ws(ws, Mq, Mk, D, dtype);
  void *P = L.P, *Vt = L.Vt;
  float *mstat = L.mstat, *lstat = L.lstat, *partial = L.partial;
  const bool split = dtype == HVR_F16S;
  const bool strides_ok = split ? (gsq % 32 == 0 && gsk % 32 == 0 && gsv % 32 == 0 && gso % 32 == 0)
                                : (two_byte && gsq % 8 == 0 && gsk % 8 == 0 && gsv % 8 == 0 && gso % 8 == 0);
  if (split && (ldv % 64 || !aligned128(V) || ldo % 32 || !aligned128(O) || D % 64)) return fail(HVR_EINVAL, "split-half relation: D, ldv multiples of 64, ldo of 32, 128-byte aligned V / O");
  if (split && split_normalizes(Mq)) {
    const int rc = normalize_blocks_ok(Mk, "split-half relation");
    if (rc) return rc;
  }
  // (exact: "bit for bit hvr_relation_fwd's" only holds when the single call takes the SAME scores kernel -- a per-group tile count
  // the one-group rule sends to the tile engine, e.g. Mq = Mk = 5 400: 352 tiles, runs as per-group single calls)
  // ---- few query rows (the key stage, hrnmp_bbox_head.py:269-278,888-891: 300 x 4 500 per clip), two-byte operands: ONE launch per pass
  // over all groups -- the tile engine's batch dimension (GemmParams::batch, gridDim.z = group): scores + V^T (the transposing workgroups
  // behind every group's score tiles), the key-sliced apply pass, one reduce.  Every group's arithmetic is hvr_relation_fwd's (same
  // tiles, same slices, same order): bit-identical to G single calls, in one sixth of the launches.  VERDICT r05 item 4.
  const int key_slices = apply_slices(Mq, Mk, D);
  if (groups > 1 && mode != 0 && staging && strides_ok && two_byte && Mq <= 1024 && key_slices > 1 && D % 8 == 0 && ldv % 8 == 0 &&
      ldo % 8 == 0 && aligned16(V) && aligned16(Vt) && aligned16(O) && per % 16 == 0 &&
      !scores_bt_supported(Mq, Mk, D, ldq, ldk, ldv, ldp, Q, K, V, P, Vt, 1, false)) {
    GemmParams p;
    int rc = fill_linear(p, Q, K, P, Mq, (Mk + 3) / 4 * 4, D, ldq, ldk, ldp, dtype, staging);
    if (rc) return rc;
    p.batch = groups;
    p.gs_a = gsq * (long)es; p.gs_b = gsk * (long)es; p.gs_c = (long)per; p.gs_stat = (long)(per / 4);
    p.tr_in = V; p.tr_out = Vt; p.tr_R = Mk; p.tr_C = D; p.tr_ldx = ldv; p.tr_ldt = ldp;
    p.gs_tr_in = gsv * (long)es; p.gs_tr_out = (long)per;
    const int score_tiles = ((Mq + 127) / 128) * ((Mk + 127) / 128);
    const int vt_tiles = ((D + 63) / 64) * (int)((ldp + 63) / 64);
    // transposing workgroups per group: together with the score tiles of all groups about two rounds of the chip's 512 resident
    // workgroups (128 x 128 tiles, two per CU); at least 32, at most one per 64 x 64 tile
    int nb = (1024 - groups * score_tiles) / groups;
    nb = nb < 32 ? 32 : nb;
    p.tr_blocks = nb < vt_tiles ? nb : vt_tiles;
    p.N = Mk;
    p.scale = scale; p.mstat = mstat; p.lstat = lstat; p.ntile = nt;
    // the double-buffered 128 x 128 shape (two workgroups per CU: the 1 024 workgroups of four clips are two rounds) -- the single call's
    // four-stage ring holds one workgroup per CU and is the better latency chain for ONE clip's 108 tiles; same MFMA order, same P~
    // (sweep: 112 us per four clips against 122; profiles/r06_key_stage.txt)
    p.tile_hint = 1; p.group_m = 8;
    rc = check_launch(run_tile_op(p, EPI_SCORES, s), "relation (grouped key stage): scores");
    if (rc) return rc;
    GemmParams a;
    rc = fill_linear(a, P, Vt, O, Mq, D, (int)ldp, ldp, ldp, ldo, dtype, staging);
    if (rc) return rc;
    a.mstat = mstat; a.lstat = lstat; a.ntile = nt; a.group_m = 1;
    a.batch = groups; a.gs_a = (long)per; a.gs_b = (long)per; a.gs_c = (long)per; a.gs_stat = (long)(per / 4);
    const int per_blk = apply_slice_blocks();
    a.ksplit_steps = per_blk * 2; a.ksplit_count = key_slices; a.csplit_bytes = (long)Mq * D * 4;
    a.C = partial; a.ldc = D; a.out_f32 = 1; a.tile_hint = 1;
    hipError_t e = run_tile_op(a, EPI_APPLY, s);
    if (e == hipSuccess) e = run_splitk_reduce_half_batched(partial, O, Mq, D, ldo, key_slices, dtype == HVR_F16, groups, (long)(per / 4), gso, s);
    return check_launch(e, "relation (grouped key stage): apply");
  }
  // the same stage on split-half operands: the scores pass and the folded apply pass (relation_split_tail's form for few query rows) as one
  // launch each over all groups, the V^T copies per group in between -- 24 apply tiles per clip are 96 on the chip at once
  if (groups > 1 && mode != 0 && staging && strides_ok && split && Mq < 1024 &&
      !scores_bt_supported(Mq, Mk, D, ldq, ldk, ldv, ldp, Q, K, V, P, Vt, 1, true)) {
    GemmParams p;
    int rc = fill_linear(p, Q, K, P, Mq, (Mk + 3) / 4 * 4, D, ldq, ldk, ldp, dtype, staging);
    if (rc) return rc;
    p.N = Mk; p.scale = scale; p.mstat = mstat; p.lstat = lstat; p.ntile = nt; p.group_m = 8; p.tile_hint = 0;
    p.batch = groups; p.gs_a = gsq * (long)es; p.gs_b = gsk * (long)es; p.gs_c = (long)per; p.gs_stat = (long)(per / 4);
    rc = check_launch(run_tile_op(p, EPI_SCORES, s), "relation (grouped key stage, split half): scores");
    if (rc) return rc;
    for (int g = 0; g < groups; ++g) {
      rc = check_launch(run_transpose_pad((const char*)V + (size_t)g * gsv * es, (char*)Vt + (size_t)g * per, Mk, D, ldv, ldp, HVR_F16S, s),
                        "relation (grouped key stage, split half): V transpose");
      if (rc) return rc;
    }
    GemmParams a;
    rc = fill_linear(a, P, Vt, O, Mq, D, (int)ldp, ldp, ldp, ldo, HVR_F16S, staging);
    if (rc) return rc;
    a.alpha = 1.f / kSplitProbScale;
    a.mstat = mstat; a.lstat = lstat; a.ntile = nt; a.tile_hint = 0;
    a.batch = groups; a.gs_a = (long)per; a.gs_b = (long)per; a.gs_c = gso * (long)es; a.gs_stat = (long)(per / 4);
    return check_launch(run_tile_op(a, EPI_APPLY, s), "relation (grouped key stage, split half): apply");
  }
  if (groups == 1 || mode == 0 || !staging || !strides_ok ||
      !scores_bt_supported(Mq, Mk, D, ldq, ldk, ldv, ldp, Q, K, V, P, Vt, groups, split) ||
      (exact && !scores_bt_supported(Mq, Mk, D, ldq, ldk, ldv, ldp, Q, K, V, P, Vt, 1, split))) {
    for (int g = 0; g < groups; ++g) {
      const int rc = hvr_relation_fwd((const char*)Q + (size_t)g * gsq * es, ldq, (const char*)K + (size_t)g * gsk * es, ldk,
                                      (const char*)V + (size_t)g * gsv * es, ldv, (char*)O + (size_t)g * gso * es, ldo, Mq, Mk, D, scale,
                                      dtype, staging, (char*)ws + (size_t)g * per, per, stream);
      if (rc) return rc;
    }
    return HVR_OK;
  }
  // exact: every group's result is hvr_relation_fwd's bit for bit (one scores launch over all groups, its arithmetic per tile
  // unchanged; the apply pass per group) -- what the batched head's equality tests run
  const bool bt_apply = !exact && mode >= 2 && (two_byte || split) && apply_bt_supported(Mq, Mk, D, ldp, ldo, P, Vt, O, groups, split);
  const ScoresBTParams b = scores_bt_params(Q, ldq, K, ldk, V, ldv, L, Mq, Mk, D, scale, dtype, groups, gsq, gsk, gsv, per, bt_apply ? 1 : 0);
  int rc = check_launch(run_scores_bt(b, s), "relation (grouped): scores");
  if (rc) return rc;
  if (bt_apply) {
    ApplyBTParams a;
    a.P = (const bf16_t*)P; a.Vt = (const bf16_t*)Vt; a.mstat = mstat; a.lstat = lstat; a.O = (bf16_t*)O;
    a.Mq = Mq; a.D = D; a.ntile = nt; a.ldp = ldp; a.ldo = ldo; a.groups = groups;
    a.gs_p = b.gs_p; a.gs_vt = b.gs_vt; a.gs_stat = b.gs_stat; a.gs_o = gso; a.split = split ? 1 : (dtype == HVR_F16 ? 2 : 0);
    return check_launch(run_apply_bt(a, s), "relation (grouped): apply");
  }
  for (int g = 0; g < groups; ++g) {
    const RelationWs G = relation_ws((char*)ws + (size_t)g * per, Mq, Mk, D, dtype);
    if (split) {   // one persistent scores launch over all groups (V^T included); the normalising sweep and the product per group
      rc = relation_split_tail(G.P, G.Vt, G.mstat, G.lstat, nullptr, ldv, (char*)O + (size_t)g * gso * es, ldo, Mq, Mk, D, ldp, nt, staging, s);
      if (rc) return rc;
      continue;
    }
    rc = relation_apply_pass(G.P, G.Vt, G.mstat, G.lstat, G.partial, (char*)O + (size_t)g * gso * es, ldo, Mq, Mk, D, ldp, nt, dtype, staging, s);
    if (rc) return rc;
  }
  return HVR_OK;
}

// ---- relation backward (attention backward of one stage) ----
struct RelationProbsWs { float *mstat, *lstat; size_t bytes; };   // [Mq][ntile] each
static RelationProbsWs relation_probs_ws(void* base, int Mq, int Mk) {
  const long nt = rel_ldp(Mk) / 128;
  Carver c(base);
  RelationProbsWs L;
  L.mstat = c.take<float>((size_t)Mq * nt);
  L.lstat = c.take<float>((size_t)Mq * nt);
  L.bytes = c.off;
  return L;
}
size_t hvr_relation_probs_workspace_bytes(int Mq, int Mk) { return relation_probs_ws(nullptr, Mq, Mk).bytes; }

int hvr_relation_probs(const void* Q, int64_t ldq, const void* K, int64_t ldk, void* P, int64_t ldp, int Mq, int Mk, int D,
                       float scale, int dtype, int staging, void* ws, size_t ws_bytes, void* stream) {
  if (!Q || !K || !P || !ws) return fail(HVR_EINVAL, "null pointer");
  if (Mq <= 0 || Mk <= 0) return fail(HVR_EINVAL, "empty relation Mq=%d Mk=%d", Mq, Mk);
  if (!(scale > 0.f)) return fail(HVR_EINVAL, "relation scale must be positive, got %g", (double)scale);
  if (ldp != rel_ldp(Mk)) return fail(HVR_EINVAL, "P rows must be %ld elements (keys padded to 128), got %ld", rel_ldp(Mk), (long)ldp);
  if (int rc = normalize_blocks_ok(Mk, "relation probs")) return rc;
  if (ws_bytes < hvr_relation_probs_workspace_bytes(Mq, Mk)) return fail(HVR_EWORKSPACE, "relation probs workspace too small");
  const int nt = (int)(ldp / 128);
  const RelationProbsWs L = relation_probs_ws(ws, Mq, Mk);
  float *mstat = L.mstat, *lstat = L.lstat;
  hipStream_t s = (hipStream_t)stream;
  GemmParams p;
  int rc = fill_linear(p, Q, K, P, Mq, (Mk + 3) / 4 * 4, D, ldq, ldk, ldp, dtype, staging);
  if (rc) return rc;
  p.N = Mk;
  p.scale = scale; p.mstat = mstat; p.lstat = lstat; p.ntile = nt; p.group_m = 8;
  rc = check_launch(run_tile_op(p, EPI_SCORES, s), "relation probs: scores");
  if (rc) return rc;
  return check_launch(run_relation_normalize(P, mstat, lstat, Mq, nt, ldp, dtype, 1.f / kSplitProbScale, s), "relation probs: normalise");
}

int hvr_relation_dscore(const void* P, const void* dP, const void* dO, int64_t ldgo, const void* O, int64_t ldo, void* dS,
                        int Mq, int64_t ldp, int D, float scale, int dtype, void* stream) {
  if (!P || !dP || !dO || !O || !dS) return fail(HVR_EINVAL, "null pointer");
  if (Mq <= 0 || D <= 0 || D % 4 || ldp % 4 || ldgo % 4 || ldo % 4) return fail(HVR_EINVAL, "bad relation dscore shape");
  return check_launch(run_relation_dscore(P, dP, dO, O, dS, Mq, ldp, D, ldgo, ldo, scale, dtype, (hipStream_t)stream),
                      "hvr_relation_dscore");
}

int hvr_im2col_nhwc(const void* x, void* cols, int B, int H, int W, int Cin, int KH, int KW, int pad, int dil, int dtype, void* stream) {
  if (!x || !cols || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % 4 || KH <= 0 || KW <= 0 || pad < 0 || dil <= 0)
    return fail(HVR_EINVAL, "bad im2col arguments (Cin %% 4 == 0 required)");
  const int OH = H + 2 * pad - dil * (KH - 1), OW = W + 2 * pad - dil * (KW - 1);
  if (OH <= 0 || OW <= 0) return fail(HVR_EINVAL, "empty im2col output");
  return check_launch(run_im2col_nhwc(x, cols, B, H, W, Cin, KH, KW, pad, dil, OH, OW, dtype, (hipStream_t)stream), "hvr_im2col_nhwc");
}

int hvr_im2col_t(const void* x, void* colsT, int64_t ldt, int B, int H, int W, int Cin, int KH, int KW, int pad, int dil, int dtype, void* stream) {
  if (!x || !colsT || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % 8 || KH <= 0 || KW <= 0 || pad < 0 || dil <= 0)
    return fail(HVR_EINVAL, "bad im2col_t arguments (Cin %% 8 == 0 required)");
  if (dtype != HVR_BF16 && dtype != HVR_F16) return fail(HVR_EUNSUPPORTED, "hvr_im2col_t takes bf16 / half maps (f32: hvr_im2col_nhwc + hvr_transpose_pad)");
  const int OH = H + 2 * pad - dil * (KH - 1), OW = W + 2 * pad - dil * (KW - 1);
  if (OH <= 0 || OW <= 0) return fail(HVR_EINVAL, "empty im2col output");
  if (ldt % 8 || ldt < (int64_t)B * OH * OW || !aligned16(x) || !aligned16(colsT)) return fail(HVR_EINVAL, "im2col_t: ldt a multiple of 8 >= B*OH*OW, 16-byte aligned buffers");
  return check_launch(run_im2col_t(x, colsT, B, H, W, Cin, KH, KW, pad, dil, OH, OW, (long)ldt, (hipStream_t)stream), "hvr_im2col_t");
}

int hvr_relu_bwd_t(const void* dY, const void* Y, void* dZ, void* dZt, int64_t ldt, int R, int C, int dtype, void* stream) {
  if (!dY || !Y || !dZ || !dZt || R <= 0 || C <= 0 || C % 8 || ldt % 8 || ldt < R) return fail(HVR_EINVAL, "bad relu_bwd_t arguments (C %% 8 == 0, ldt %% 8 == 0, ldt >= R)");
  if (dtype != HVR_BF16 && dtype != HVR_F16) return fail(HVR_EUNSUPPORTED, "hvr_relu_bwd_t takes bf16 / half maps (f32: hvr_relu_bwd + hvr_transpose_pad)");
  if (!aligned16(dY) || !aligned16(Y) || !aligned16(dZ) || !aligned16(dZt)) return fail(HVR_EINVAL, "relu_bwd_t: 16-byte aligned buffers");
  return check_launch(run_relu_bwd_t(dY, Y, dZ, dZt, R, C, (long)ldt, (hipStream_t)stream), "hvr_relu_bwd_t");
}

int hvr_scale_rows(const void* w, const float* scale, void* out, int R, int64_t C, int dtype, void* stream) {
  if (!w || !scale || !out || R <= 0 || C <= 0 || C % 4) return fail(HVR_EINVAL, "bad scale_rows arguments (C %% 4 == 0 required)");
  return check_launch(run_scale_rows(w, scale, out, R, C, dtype, (hipStream_t)stream), "hvr_scale_rows");
}

size_t hvr_sgd_workspace_bytes(void) { return sgd_workspace_bytes(); }

// ---- head training helpers ----
int hvr_relu_bwd(const void* dY, const void* Y, void* dZ, int64_t n, int dtype, void* stream) {
  if (n == 0) return HVR_OK;
  if (!dY || !Y || !dZ || n < 0 || n % 4) return fail(HVR_EINVAL, "bad relu_bwd arguments (n %% 4 == 0 required)");
  return check_launch(run_relu_bwd(dY, Y, dZ, n, dtype, (hipStream_t)stream), "hvr_relu_bwd");
}

size_t hvr_colsum_workspace_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  const int s = colsum_slices(M, N);
  return s > 1 ? (size_t)s * N * sizeof(float) : 0;
}

int hvr_colsum(const void* dY, float* db, int M, int N, int64_t ld, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (!dY || !db || M <= 0 || N <= 0) return fail(HVR_EINVAL, "bad colsum arguments");
  const size_t need = hvr_colsum_workspace_bytes(M, N);
  if (need && (!ws || ws_bytes < need)) return fail(HVR_EWORKSPACE, "colsum workspace too small");
  return check_launch(run_colsum(dY, db, M, N, ld, dtype, (float*)ws, (hipStream_t)stream), "hvr_colsum");
}

int hvr_pack_conv_weight(const float* w, const float* scale, void* out, int Cout, int Cin, int KH, int KW, int out_dtype, void* stream) {
  if (!w || !scale || !out || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return fail(HVR_EINVAL, "bad pack_conv_weight arguments");
  if (out_dtype != HVR_F32 && out_dtype != HVR_BF16 && out_dtype != HVR_F16) return fail(HVR_EINVAL, "bad dtype");
  return check_launch(run_pack_conv_weight(w, scale, out, Cout, Cin, KH * KW, out_dtype, (hipStream_t)stream), "hvr_pack_conv_weight");
}

int hvr_pack_conv_weights_multi(const hvr_pack_item* items_dev, int n, int64_t total, int out_dtype, void* stream) {
  if (!items_dev || n <= 0 || total <= 0) return fail(HVR_EINVAL, "bad pack_conv_weights_multi arguments");
  if (out_dtype != HVR_BF16 && out_dtype != HVR_F16) return fail(HVR_EUNSUPPORTED, "hvr_pack_conv_weights_multi writes bf16 / half operands");
  return check_launch(run_pack_conv_weights_multi(items_dev, n, (long)total, out_dtype, (hipStream_t)stream), "hvr_pack_conv_weights_multi");
}

int hvr_transpose_multi(const hvr_transpose_item* items_dev, int n, int tiles, void* stream) {
  if (!items_dev || n <= 0 || tiles <= 0) return fail(HVR_EINVAL, "bad transpose_multi arguments");
  return check_launch(run_transpose_multi(items_dev, n, tiles, (hipStream_t)stream), "hvr_transpose_multi");
}

int hvr_unpack_conv_wgrads_multi(const hvr_unpack_item* items_dev, int n, int64_t total, int accumulate, void* stream) {
  if (!items_dev || n <= 0 || total <= 0) return fail(HVR_EINVAL, "bad unpack_conv_wgrads_multi arguments");
  return check_launch(run_unpack_conv_wgrads_multi(items_dev, n, (long)total, accumulate, (hipStream_t)stream), "hvr_unpack_conv_wgrads_multi");
}

int hvr_unpack_conv_wgrad(const float* dw, const float* scale, float* out, int Cout, int Cin, int KH, int KW, int accumulate, void* stream) {
  if (!dw || !scale || !out || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return fail(HVR_EINVAL, "bad unpack_conv_wgrad arguments");
  return check_launch(run_unpack_conv_wgrad(dw, scale, out, Cout, Cin, KH * KW, accumulate, (hipStream_t)stream), "hvr_unpack_conv_wgrad");
}

int hvr_det_loss(const float* logits, int ldl, int cls_off, int reg_off, int ncls, const int64_t* labels, const float* label_weights,
                 const float* bbox_targets, const float* bbox_weights, int R, float beta, float w_cls, float w_bbox, float* out3,
                 float* dlogits, void* stream) {
  if (!logits || !labels || !label_weights || !bbox_targets || !bbox_weights || !out3 || !dlogits) return fail(HVR_EINVAL, "null pointer");
  if (R <= 0 || ncls <= 1 || cls_off < 0 || reg_off < 0 || cls_off + ncls > ldl || reg_off + 4 > ldl || !(beta > 0.f))
    return fail(HVR_EINVAL, "bad det_loss shape");
  return check_launch(run_det_loss(logits, ldl, cls_off, reg_off, ncls, (const long long*)labels, label_weights, bbox_targets,
                                   bbox_weights, R, beta, w_cls, w_bbox, out3, dlogits, nullptr, (hipStream_t)stream),
                      "hvr_det_loss");
}

int hvr_det_loss_sampled(const float* logits, int ldl, int cls_off, int reg_off, int ncls, const int64_t* labels,
                         const float* label_weights, const float* bbox_targets, const float* bbox_weights, int R,
                         const int32_t* sel_counts, float beta, float* out3, float* dlogits, void* stream) {
  if (!logits || !labels || !label_weights || !bbox_targets || !bbox_weights || !out3 || !dlogits || !sel_counts)
    return fail(HVR_EINVAL, "null pointer");
  if (R <= 0 || ncls <= 1 || cls_off < 0 || reg_off < 0 || cls_off + ncls > ldl || reg_off + 4 > ldl || !(beta > 0.f))
    return fail(HVR_EINVAL, "bad det_loss shape");
  return check_launch(run_det_loss(logits, ldl, cls_off, reg_off, ncls, (const long long*)labels, label_weights, bbox_targets,
                                   bbox_weights, R, beta, 1.f, 1.f, out3, dlogits, sel_counts, (hipStream_t)stream),
                      "hvr_det_loss_sampled");
}

size_t hvr_max_iou_assign_workspace_bytes(int n, int k) { return n > 0 && k > 0 ? assign_workspace_bytes(n, k) : 0; }

int hvr_max_iou_assign(const float* boxes, int ldb, int n, const float* gts, int k, const uint8_t* valid, float pos_iou_thr,
                       float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int64_t* gt_inds, float* max_overlaps, void* ws,
                       size_t ws_bytes, void* stream) {
  if (!boxes || !gts || !gt_inds || !max_overlaps || !ws) return fail(HVR_EINVAL, "null pointer");
  if (n <= 0 || k <= 0) return fail(HVR_EINVAL, "No gt or bboxes");  // max_iou_assigner.py:77-78 raises ValueError
  if (k > 256) return fail(HVR_EUNSUPPORTED, "at most 256 ground-truth boxes per assignment (got %d)", k);
  if (ldb < 4) return fail(HVR_EINVAL, "boxes need 4 coordinates per row");
  if (ws_bytes < assign_workspace_bytes(n, k)) return fail(HVR_EINVAL, "assign workspace too small");
  return check_launch(run_max_iou_assign(boxes, ldb, n, gts, k, valid, pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou,
                                         (long long*)gt_inds, max_overlaps, ws, (hipStream_t)stream),
                      "hvr_max_iou_assign");
}

int hvr_sample_pos_neg(const int64_t* cls, const float* keys, int n, int num, int num_expected_pos, double neg_pos_ub, int64_t* inds,
                       int32_t* counts, void* stream) {
  if (!cls || !keys || !inds || !counts) return fail(HVR_EINVAL, "null pointer");
  if (n <= 0 || num <= 0 || num_expected_pos < 0 || num_expected_pos > num) return fail(HVR_EINVAL, "bad sampler sizes");
  return check_launch(run_sample((const long long*)cls, keys, n, num, num_expected_pos, neg_pos_ub, (long long*)inds, counts,
                                 (hipStream_t)stream),
                      "hvr_sample_pos_neg");
}

int hvr_box_targets(const float* boxes, int ldb, int n, const float* gts, const int64_t* gt_labels, const int64_t* gt_inds,
                    const int64_t* inds, const int32_t* counts, int num, const float* means4, const float* stds4, float pos_weight,
                    int scatter, int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights, void* stream) {
  if (!boxes || !gts || !gt_inds || !inds || !counts || !means4 || !stds4 || !labels || !label_weights || !bbox_targets || !bbox_weights)
    return fail(HVR_EINVAL, "null pointer");
  if (n <= 0 || num <= 0 || ldb < 4) return fail(HVR_EINVAL, "bad box_targets sizes");
  for (int i = 0; i < 4; ++i)
    if (stds4[i] == 0.f) return fail(HVR_EINVAL, "target_stds must be non-zero");
  return check_launch(run_box_targets(boxes, ldb, n, gts, (const long long*)gt_labels, (const long long*)gt_inds, (const long long*)inds,
                                      counts, num, means4, stds4, pos_weight, scatter, (long long*)labels, label_weights, bbox_targets,
                                      bbox_weights, (hipStream_t)stream),
                      "hvr_box_targets");
}

int hvr_rpn_loss(const float* o, int ldo, int A, int rows, const int64_t* labels, const float* label_weights, const float* bbox_targets,
                 const float* bbox_weights, const int32_t* counts, float beta, float* out2, float* d_o, void* stream) {
  if (!o || !labels || !label_weights || !bbox_targets || !bbox_weights || !counts || !out2 || !d_o) return fail(HVR_EINVAL, "null pointer");
  if (A <= 0 || rows <= 0 || ldo < 5 * A || !(beta > 0.f)) return fail(HVR_EINVAL, "bad rpn_loss shape");
  return check_launch(run_rpn_loss(o, ldo, A, rows, (const long long*)labels, label_weights, bbox_targets, bbox_weights, counts, beta,
                                   out2, d_o, (hipStream_t)stream),
                      "hvr_rpn_loss");
}

// ---- sigmoid focal loss (focal.hip; the rule: include/hvr_hip.h)
static int focal_args(const char* what, int N, int C, int ldl, float gamma, float alpha) {
  if (N < 1 || C < 1) return fail(HVR_EINVAL, "%s: N=%d rows of C=%d columns (N, C >= 1)", what, N, C);
  if (ldl < C) return fail(HVR_EINVAL, "%s: row pitch ldl=%d is below C=%d (ldl >= C)", what, ldl, C);
  if ((long)N * ldl >= (1L << 31)) return fail(HVR_EUNSUPPORTED, "%s: N * ldl = %ld elements (N * ldl < 2^31)", what, (long)N * ldl);
  if (!(gamma >= 0.f) || !std::isfinite(gamma)) return fail(HVR_EINVAL, "%s: gamma=%g (gamma >= 0)", what, (double)gamma);
  if (!(alpha >= 0.f && alpha <= 1.f)) return fail(HVR_EINVAL, "%s: alpha=%g (0 <= alpha <= 1)", what, (double)alpha);
  return HVR_OK;
}
static int focal_dtype(const char* what, int dtype) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "%s: bad dtype %d", what, dtype);
  if (dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "%s: no split-half logits (HVR_F32 / HVR_BF16 / HVR_F16)", what);
  return HVR_OK;
}
int hvr_sigmoid_focal_loss_fwd(const void* logits, int ldl, const int64_t* targets, int N, int C, float gamma, float alpha, int dtype,
                               float* loss, void* stream) {
  if (!logits || !targets || !loss) return fail(HVR_EINVAL, "hvr_sigmoid_focal_loss_fwd: null pointer");
  if (int rc = focal_dtype("hvr_sigmoid_focal_loss_fwd", dtype)) return rc;
  if (int rc = focal_args("hvr_sigmoid_focal_loss_fwd", N, C, ldl, gamma, alpha)) return rc;
  return check_launch(run_focal_elem(logits, ldl, (const long long*)targets, nullptr, N, C, gamma, alpha, dtype, loss, (hipStream_t)stream),
                      "hvr_sigmoid_focal_loss_fwd");
}
int hvr_sigmoid_focal_loss_bwd(const void* logits, int ldl, const int64_t* targets, const float* d_loss, int N, int C, float gamma,
                               float alpha, int dtype, float* d_logits, void* stream) {
  if (!logits || !targets || !d_loss || !d_logits) return fail(HVR_EINVAL, "hvr_sigmoid_focal_loss_bwd: null pointer");
  if (int rc = focal_dtype("hvr_sigmoid_focal_loss_bwd", dtype)) return rc;
  if (int rc = focal_args("hvr_sigmoid_focal_loss_bwd", N, C, ldl, gamma, alpha)) return rc;
  return check_launch(run_focal_elem(logits, ldl, (const long long*)targets, d_loss, N, C, gamma, alpha, dtype, d_logits, (hipStream_t)stream),
                      "hvr_sigmoid_focal_loss_bwd");
}
int hvr_focal_loss_splits(int N, int C) {
  if (N <= 0 || C <= 0) return 0;
  int S, rows;
  focal_split(N, C, &S, &rows);
  return S;
}
size_t hvr_focal_loss_workspace_bytes(int N, int C) { return align256((size_t)hvr_focal_loss_splits(N, C) * sizeof(float)); }
int hvr_focal_loss(const float* logits, int ldl, const int64_t* targets, const float* w, int N, int C, float gamma, float alpha,
                   float loss_weight, float avg, const int32_t* counts_dev, void* ws, size_t ws_bytes, float* out1, float* d_logits,
                   void* stream) {
  if (!logits || !targets || !ws || !out1 || !d_logits) return fail(HVR_EINVAL, "hvr_focal_loss: null pointer");
  if (int rc = focal_args("hvr_focal_loss", N, C, ldl, gamma, alpha)) return rc;
  if (!counts_dev && !(avg > 0.f && std::isfinite(avg))) return fail(HVR_EINVAL, "hvr_focal_loss: avg=%g (avg > 0 when no device count is given)", (double)avg);
  if (!std::isfinite(loss_weight)) return fail(HVR_EINVAL, "hvr_focal_loss: loss_weight=%g is not finite", (double)loss_weight);
  if (ws_bytes < hvr_focal_loss_workspace_bytes(N, C))
    return fail(HVR_EWORKSPACE, "hvr_focal_loss: workspace of %zu bytes, %zu needed (ws_bytes >= hvr_focal_loss_workspace_bytes)", ws_bytes,
                hvr_focal_loss_workspace_bytes(N, C));
  return check_launch(run_focal_fused(logits, ldl, (const long long*)targets, w, N, C, gamma, alpha, loss_weight, avg, counts_dev, (float*)ws, out1,
                                      d_logits, (hipStream_t)stream),
                      "hvr_focal_loss");
}
int hvr_rpn_focal_loss(const float* o, int ldo, int A, int rows, const int64_t* labels, const float* label_weights,
                       const float* bbox_targets, const float* bbox_weights, const int32_t* counts, float beta, float gamma, float alpha,
                       float w_cls, float w_bbox, float* out2, float* d_o, void* stream) {
  if (!o || !labels || !label_weights || !bbox_targets || !bbox_weights || !counts || !out2 || !d_o) return fail(HVR_EINVAL, "hvr_rpn_focal_loss: null pointer");
  if (A <= 0 || rows <= 0 || ldo < 5 * A || !(beta > 0.f))
    return fail(HVR_EINVAL, "hvr_rpn_focal_loss: A=%d rows=%d ldo=%d beta=%g (A, rows >= 1, ldo >= 5 A, beta > 0)", A, rows, ldo, (double)beta);
  if ((long)rows * ldo >= (1L << 31)) return fail(HVR_EUNSUPPORTED, "hvr_rpn_focal_loss: rows * ldo = %ld elements (below 2^31)", (long)rows * ldo);
  if (int rc = focal_args("hvr_rpn_focal_loss", rows, 1, ldo, gamma, alpha)) return rc;
  if (!std::isfinite(w_cls) || !std::isfinite(w_bbox)) return fail(HVR_EINVAL, "hvr_rpn_focal_loss: loss weights must be finite");
  return check_launch(run_rpn_focal_loss(o, ldo, A, rows, (const long long*)labels, label_weights, bbox_targets, bbox_weights, counts, beta, gamma,
                                         alpha, w_cls, w_bbox, out2, d_o, (hipStream_t)stream),
                      "hvr_rpn_focal_loss");
}

// ---- regression, IoU and GHM losses (reg_loss.hip, ghm.hip; the rules: include/hvr_hip.h)
static int reg_args(const char* what, int rule, int N, int D, int ldp, float beta, float alpha, float gamma, float* prm4) {
  if (rule < HVR_REG_SMOOTH_L1 || rule > HVR_REG_MSE) return fail(HVR_EINVAL, "%s: rule %d (HVR_REG_SMOOTH_L1 / _BALANCED_L1 / _MSE)", what, rule);
  if (N < 1 || D < 1) return fail(HVR_EINVAL, "%s: N=%d rows of D=%d columns (N, D >= 1)", what, N, D);
  if (ldp < D) return fail(HVR_EINVAL, "%s: row pitch ldp=%d is below D=%d (ldp >= D)", what, ldp, D);
  if ((long)N * ldp >= (1L << 31)) return fail(HVR_EUNSUPPORTED, "%s: N * ldp = %ld elements (below 2^31)", what, (long)N * ldp);
  prm4[0] = beta; prm4[1] = alpha; prm4[2] = gamma; prm4[3] = 0.f;
  if (rule != HVR_REG_MSE && !(beta > 0.f && std::isfinite(beta))) return fail(HVR_EINVAL, "%s: beta=%g (beta > 0)", what, (double)beta);
  if (rule == HVR_REG_BALANCED_L1) {
    if (!(alpha > 0.f && std::isfinite(alpha)) || !(gamma > 0.f && std::isfinite(gamma)))
      return fail(HVR_EINVAL, "%s: alpha=%g gamma=%g (alpha, gamma > 0)", what, (double)alpha, (double)gamma);
    const double b = std::exp((double)gamma / (double)alpha) - 1.0;      // formed in f64, rounded once
    if (!(b < 3e38)) return fail(HVR_EINVAL, "%s: e^(gamma / alpha) - 1 = %g does not fit f32", what, b);
    prm4[3] = (float)b;
  }
  return HVR_OK;
}
static int reduce_args(const char* what, float loss_weight, float avg, const int32_t* counts_dev, size_t ws_bytes, size_t need) {
  if (!counts_dev && !(avg > 0.f && std::isfinite(avg))) return fail(HVR_EINVAL, "%s: avg=%g (avg > 0 when no device count is given)", what, (double)avg);
  if (!std::isfinite(loss_weight)) return fail(HVR_EINVAL, "%s: loss_weight=%g is not finite", what, (double)loss_weight);
  if (ws_bytes < need) return fail(HVR_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
  return HVR_OK;
}
int hvr_reg_loss_fwd(int rule, const float* pred, int ldp, const float* target, int N, int D, float beta, float alpha, float gamma, float* loss,
                     void* stream) {
  if (!pred || !target || !loss) return fail(HVR_EINVAL, "hvr_reg_loss_fwd: null pointer");
  float prm[4];
  if (int rc = reg_args("hvr_reg_loss_fwd", rule, N, D, ldp, beta, alpha, gamma, prm)) return rc;
  return check_launch(run_reg_elem(rule, pred, ldp, target, nullptr, N, D, prm, loss, (hipStream_t)stream), "hvr_reg_loss_fwd");
}
int hvr_reg_loss_bwd(int rule, const float* pred, int ldp, const float* target, const float* d_loss, int N, int D, float beta, float alpha,
                     float gamma, float* d_pred, void* stream) {
  if (!pred || !target || !d_loss || !d_pred) return fail(HVR_EINVAL, "hvr_reg_loss_bwd: null pointer");
  float prm[4];
  if (int rc = reg_args("hvr_reg_loss_bwd", rule, N, D, ldp, beta, alpha, gamma, prm)) return rc;
  return check_launch(run_reg_elem(rule, pred, ldp, target, d_loss, N, D, prm, d_pred, (hipStream_t)stream), "hvr_reg_loss_bwd");
}
int hvr_reg_loss_splits(int N, int D) { return hvr_focal_loss_splits(N, D); }
size_t hvr_reg_loss_workspace_bytes(int N, int D) { return align256((size_t)hvr_reg_loss_splits(N, D) * sizeof(float)); }
int hvr_reg_loss(int rule, const float* pred, int ldp, const float* target, const float* w, int N, int D, float beta, float alpha, float gamma,
                 float loss_weight, float avg, const int32_t* counts_dev, void* ws, size_t ws_bytes, float* out1, float* d_pred, void* stream) {
  if (!pred || !target || !ws || !out1 || !d_pred) return fail(HVR_EINVAL, "hvr_reg_loss: null pointer");
  float prm[4];
  if (int rc = reg_args("hvr_reg_loss", rule, N, D, ldp, beta, alpha, gamma, prm)) return rc;
  if (int rc = reduce_args("hvr_reg_loss", loss_weight, avg, counts_dev, ws_bytes, hvr_reg_loss_workspace_bytes(N, D))) return rc;
  return check_launch(run_reg_fused(rule, pred, ldp, target, w, N, D, prm, loss_weight, avg, counts_dev, (float*)ws, out1, d_pred, (hipStream_t)stream),
                      "hvr_reg_loss");
}
static int box_args(const char* what, int rule, int n, float beta, float eps) {
  if (rule < HVR_BOX_IOU || rule > HVR_BOX_BOUNDED_IOU) return fail(HVR_EINVAL, "%s: rule %d (HVR_BOX_IOU / HVR_BOX_BOUNDED_IOU)", what, rule);
  if (n < 1 || n >= (1 << 29)) return fail(HVR_EINVAL, "%s: n=%d box pairs (1 <= n < 2^29)", what, n);
  if (!(eps > 0.f && std::isfinite(eps))) return fail(HVR_EINVAL, "%s: eps=%g (eps > 0)", what, (double)eps);
  if (rule == HVR_BOX_BOUNDED_IOU && !(beta > 0.f && std::isfinite(beta))) return fail(HVR_EINVAL, "%s: beta=%g (beta > 0)", what, (double)beta);
  return HVR_OK;
}
int hvr_box_loss_fwd(int rule, const float* pred, const float* target, int n, float beta, float eps, float* loss, void* stream) {
  if (!pred || !target || !loss) return fail(HVR_EINVAL, "hvr_box_loss_fwd: null pointer");
  if (int rc = box_args("hvr_box_loss_fwd", rule, n, beta, eps)) return rc;
  return check_launch(run_box_elem(rule, pred, target, nullptr, n, beta, eps, loss, (hipStream_t)stream), "hvr_box_loss_fwd");
}
int hvr_box_loss_bwd(int rule, const float* pred, const float* target, const float* d_loss, int n, float beta, float eps, float* d_pred,
                     void* stream) {
  if (!pred || !target || !d_loss || !d_pred) return fail(HVR_EINVAL, "hvr_box_loss_bwd: null pointer");
  if (int rc = box_args("hvr_box_loss_bwd", rule, n, beta, eps)) return rc;
  return check_launch(run_box_elem(rule, pred, target, d_loss, n, beta, eps, d_pred, (hipStream_t)stream), "hvr_box_loss_bwd");
}
int hvr_box_loss_splits(int n) { return hvr_focal_loss_splits(n, 4); }
size_t hvr_box_loss_workspace_bytes(int n) { return align256((size_t)hvr_box_loss_splits(n) * sizeof(float)); }
int hvr_box_loss(int rule, const float* pred, const float* target, const float* w, int n, float beta, float eps, float loss_weight, float avg,
                 const int32_t* counts_dev, void* ws, size_t ws_bytes, float* out1, float* d_pred, void* stream) {
  if (!pred || !target || !ws || !out1 || !d_pred) return fail(HVR_EINVAL, "hvr_box_loss: null pointer");
  if (int rc = box_args("hvr_box_loss", rule, n, beta, eps)) return rc;
  if (int rc = reduce_args("hvr_box_loss", loss_weight, avg, counts_dev, ws_bytes, hvr_box_loss_workspace_bytes(n))) return rc;
  return check_launch(run_box_fused(rule, pred, target, w, n, beta, eps, loss_weight, avg, counts_dev, (float*)ws, out1, d_pred, (hipStream_t)stream),
                      "hvr_box_loss");
}
static int ghm_args(const char* what, int N, int C, int bins, float momentum, const float* acc_sum, float loss_weight, size_t ws_bytes) {
  if (N < 1 || C < 1 || (long)N * C >= (1L << 31)) return fail(HVR_EINVAL, "%s: N=%d x C=%d elements (N, C >= 1, N C < 2^31)", what, N, C);
  if (bins < 1 || bins > 64) return fail(HVR_EINVAL, "%s: bins=%d (1 .. 64)", what, bins);
  if (!(momentum >= 0.f && momentum < 1.f)) return fail(HVR_EINVAL, "%s: momentum=%g (0 <= momentum < 1)", what, (double)momentum);
  if (momentum > 0.f && !acc_sum) return fail(HVR_EINVAL, "%s: momentum > 0 needs the acc_sum buffer", what);
  if (!std::isfinite(loss_weight)) return fail(HVR_EINVAL, "%s: loss_weight=%g is not finite", what, (double)loss_weight);
  if (ws_bytes < hvr_ghm_workspace_bytes(N, C))
    return fail(HVR_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (ws_bytes >= hvr_ghm_workspace_bytes)", what, ws_bytes, hvr_ghm_workspace_bytes(N, C));
  return HVR_OK;
}
int hvr_ghm_splits(int N, int C) {
  if (N <= 0 || C <= 0) return 0;
  int S;
  long per;
  ghm_split(N, C, &S, &per);
  return S;
}
size_t hvr_ghm_workspace_bytes(int N, int C) { return N <= 0 || C <= 0 ? 0 : align256(ghm_workspace_words(N, C) * 4); }
int hvr_ghmc_loss(const float* logits, const float* target, const int64_t* labels, const float* weight, int weight_per_row, int N, int C,
                  const float* edges, int bins, float momentum, float* acc_sum, float loss_weight, void* ws, size_t ws_bytes, float* out1,
                  float* d_logits, void* stream) {
  if (!logits || !weight || !edges || !ws || !out1 || !d_logits) return fail(HVR_EINVAL, "hvr_ghmc_loss: null pointer");
  if (!target == !labels) return fail(HVR_EINVAL, "hvr_ghmc_loss: exactly one of target (f32 [N][C]) and labels (int64 [N])");
  if (int rc = ghm_args("hvr_ghmc_loss", N, C, bins, momentum, acc_sum, loss_weight, ws_bytes)) return rc;
  return check_launch(run_ghmc(logits, target, (const long long*)labels, weight, weight_per_row ? 1 : 0, N, C, edges, bins, momentum, acc_sum,
                               loss_weight, ws, out1, d_logits, (hipStream_t)stream),
                      "hvr_ghmc_loss");
}
int hvr_ghmr_loss(const float* pred, const float* target, const float* weight, int N, int C, float mu, const float* edges, int bins,
                  float momentum, float* acc_sum, float loss_weight, void* ws, size_t ws_bytes, float* out1, float* d_pred, void* stream) {
  if (!pred || !target || !weight || !edges || !ws || !out1 || !d_pred) return fail(HVR_EINVAL, "hvr_ghmr_loss: null pointer");
  if (!(mu > 0.f && std::isfinite(mu))) return fail(HVR_EINVAL, "hvr_ghmr_loss: mu=%g (mu > 0)", (double)mu);
  if (int rc = ghm_args("hvr_ghmr_loss", N, C, bins, momentum, acc_sum, loss_weight, ws_bytes)) return rc;
  return check_launch(run_ghmr(pred, target, weight, N, C, mu, edges, bins, momentum, acc_sum, loss_weight, ws, out1, d_pred, (hipStream_t)stream),
                      "hvr_ghmr_loss");
}

int hvr_mining_argreduce(const float* aff, int Mq, int Mk, int64_t ld, const int64_t* labels, const int64_t* all_labels, int64_t* out4,
                         void* stream) {
  if (!aff || !labels || !all_labels || !out4) return fail(HVR_EINVAL, "null pointer");
  if (Mq <= 0 || Mk <= 0 || ld < Mk) return fail(HVR_EINVAL, "bad mining shape");
  return check_launch(run_mining_argreduce(aff, Mq, Mk, ld, (const long long*)labels, (const long long*)all_labels, (long long*)out4,
                                           (hipStream_t)stream),
                      "hvr_mining_argreduce");
}

int hvr_triplet_margin(const void* q, int64_t ldq, const void* k, int64_t ldk, int D, int Mq, int Mk, const int64_t* anchor_idx,
                       const int64_t* pos_idx, const int64_t* neg_idx, int n, float margin, int dtype, float* ws, size_t ws_bytes,
                       float* out2, float* dq, float* dk, void* stream) {
  if (!q || !k || !anchor_idx || !pos_idx || !neg_idx || !ws || !out2) return fail(HVR_EINVAL, "null pointer");
  if (D <= 0 || Mq <= 0 || Mk <= 0 || n <= 0 || ldq < D || ldk < D) return fail(HVR_EINVAL, "bad triplet shape");
  if (dtype != HVR_F32 && dtype != HVR_BF16) return fail(HVR_EINVAL, "bad dtype");
  if (ws_bytes < (size_t)n * 3 * sizeof(float)) return fail(HVR_EWORKSPACE, "triplet workspace too small");
  return check_launch(run_triplet_margin(q, ldq, k, ldk, D, Mq, Mk, (const long long*)anchor_idx, (const long long*)pos_idx,
                                         (const long long*)neg_idx, n, margin, dtype == HVR_BF16, ws, out2, dq, dk, (hipStream_t)stream),
                      "hvr_triplet_margin");
}

int hvr_ingest_frame_flip(const uint8_t* src, int src_h, int src_w, int64_t src_pitch, float* dst, int new_h, int new_w, int pad_h, int pad_w,
                          const float* mean3, const float* std3, int to_rgb, int flip, void* stream) {
  if (!src || !dst || !mean3 || !std3) return fail(HVR_EINVAL, "null pointer");
  if (src_h <= 0 || src_w <= 0 || new_h <= 0 || new_w <= 0 || pad_h < new_h || pad_w < new_w || src_pitch < 3L * src_w)
    return fail(HVR_EINVAL, "bad ingest shape");
  for (int c = 0; c < 3; ++c)
    if (std3[c] == 0.f) return fail(HVR_EINVAL, "std must be non-zero");
  return check_launch(run_ingest(src, src_h, src_w, src_pitch, dst, new_h, new_w, pad_h, pad_w, mean3, std3, to_rgb, flip != 0, (hipStream_t)stream),
                      "hvr_ingest_frame_flip");
}

int hvr_ingest_frame(const uint8_t* src, int src_h, int src_w, int64_t src_pitch, float* dst, int new_h, int new_w, int pad_h, int pad_w,
                     const float* mean3, const float* std3, int to_rgb, void* stream) {
  return hvr_ingest_frame_flip(src, src_h, src_w, src_pitch, dst, new_h, new_w, pad_h, pad_w, mean3, std3, to_rgb, 0, stream);
}

// ---- test-time augmentation: box plumbing ----
static int tta_check_augs(int A, const float* img_w, const float* scale_factor, const int32_t* flip) {
  if (!img_w || !scale_factor || !flip) return fail(HVR_EINVAL, "null pointer");
  if (A <= 0 || A > 16) return fail(HVR_EUNSUPPORTED, "1 <= augmentations <= 16, got %d", A);
  for (int a = 0; a < A; ++a)
    if (!(scale_factor[a] > 0.f) || !(img_w[a] > 0.f)) return fail(HVR_EINVAL, "augmentation %d: scale_factor and img_w must be positive", a);
  return HVR_OK;
}

size_t hvr_merge_aug_proposals_workspace_bytes(int A, int T, int mx) {
  return (A > 0 && T > 0 && mx > 0 && (long)A * mx <= 8192) ? tta_merge_proposals_workspace_bytes(A, T, mx) : 0;
}

int hvr_merge_aug_proposals(const float* proposals, const int32_t* counts, int A, int T, int mx, const float* img_w,
                            const float* scale_factor, const int32_t* flip, float nms_thr, int max_num, float* merged,
                            int32_t* merged_counts, void* ws, size_t ws_bytes, void* stream) {
  if (!proposals || !counts || !merged || !merged_counts || !ws) return fail(HVR_EINVAL, "null pointer");
  if (int rc = tta_check_augs(A, img_w, scale_factor, flip)) return rc;
  if (T <= 0 || mx <= 0 || max_num <= 0) return fail(HVR_EINVAL, "bad merge_aug_proposals shape");
  if ((long)A * mx > 8192) return fail(HVR_EUNSUPPORTED, "hvr_merge_aug_proposals supports A * mx <= 8192, got %ld", (long)A * mx);
  if (max_num > 4096) return fail(HVR_EUNSUPPORTED, "hvr_merge_aug_proposals supports max_num <= 4096, got %d", max_num);
  if (ws_bytes < hvr_merge_aug_proposals_workspace_bytes(A, T, mx)) return fail(HVR_EWORKSPACE, "merge_aug_proposals workspace too small");
  return check_launch(run_tta_merge_proposals(proposals, counts, A, T, mx, img_w, scale_factor, flip, nms_thr, max_num, merged,
                                              merged_counts, ws, (hipStream_t)stream),
                      "hvr_merge_aug_proposals");
}

int hvr_map_aug_rois(const float* merged, int A, int T, int max_num, const float* img_w, const float* scale_factor, const int32_t* flip,
                     float* rois, void* stream) {
  if (!merged || !rois) return fail(HVR_EINVAL, "null pointer");
  if (int rc = tta_check_augs(A, img_w, scale_factor, flip)) return rc;
  if (T <= 0 || max_num <= 0 || (long)T * max_num > (1L << 24)) return fail(HVR_EINVAL, "bad map_aug_rois shape");
  return check_launch(run_tta_map_rois(merged, A, T, max_num, img_w, scale_factor, flip, rois, (hipStream_t)stream), "hvr_map_aug_rois");
}

int hvr_merge_aug_dets(const float* boxes, const float* scores, int A, int R, int ncls, const float* img_w, const float* scale_factor,
                       const int32_t* flip, float* merged_boxes, float* merged_scores, void* stream) {
  if (R == 0) return HVR_OK;
  if (!boxes || !scores || !merged_boxes || !merged_scores) return fail(HVR_EINVAL, "null pointer");
  if (int rc = tta_check_augs(A, img_w, scale_factor, flip)) return rc;
  if (R < 0 || ncls <= 0 || (long)R * (4 + ncls) > (1L << 30)) return fail(HVR_EINVAL, "bad merge_aug_dets shape");
  return check_launch(run_tta_merge_dets(boxes, scores, A, R, ncls, img_w, scale_factor, flip, merged_boxes, merged_scores,
                                         (hipStream_t)stream),
                      "hvr_merge_aug_dets");
}

int hvr_ce_rows(const float* logits, int ldl, int cls_off, int ncls, const int64_t* labels, int R, float* loss, void* stream) {
  if (!logits || !labels || !loss) return fail(HVR_EINVAL, "null pointer");
  if (R <= 0 || ncls <= 1 || cls_off < 0 || cls_off + ncls > ldl) return fail(HVR_EINVAL, "bad ce_rows shape");
  return check_launch(run_ce_rows(logits, ldl, cls_off, ncls, (const long long*)labels, R, loss, (hipStream_t)stream), "hvr_ce_rows");
}

int hvr_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                 float grad_scale, float max_norm, float* ws, size_t ws_bytes, int first_step, void* stream) {
  if (n == 0) return HVR_OK;
  if (!param || !grad || !momentum_buf || !ws || n < 0) return fail(HVR_EINVAL, "bad sgd_step arguments");
  if (ws_bytes < hvr_sgd_workspace_bytes()) return fail(HVR_EWORKSPACE, "sgd workspace too small");
  return check_launch(run_sgd_step(param, grad, momentum_buf, n, lr, momentum, weight_decay, grad_scale, max_norm, ws, first_step,
                                   (hipStream_t)stream),
                      "hvr_sgd_step");
}

// ---- RoIAlign ----
int hvr_roi_align_fwd(const void* feat, const float* rois, void* out, int B, int C, int H, int W, int K, int PH, int PW,
                      float spatial_scale, int sample_num, int dtype, int layout, void* stream) {
  if (K == 0) return HVR_OK;
  if (!feat || !rois || !out) return fail(HVR_EINVAL, "null pointer");
  if (K < 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || PH <= 0 || PW <= 0) return fail(HVR_EINVAL, "bad roi_align shape");
  if (layout != HVR_LAYOUT_NCHW && layout != HVR_LAYOUT_NHWC) return fail(HVR_EINVAL, "bad layout %d", layout);
  return check_launch(run_roi_align_fwd(feat, rois, out, B, C, H, W, K, PH, PW, spatial_scale, sample_num, dtype, layout,
                                        (hipStream_t)stream),
                      "hvr_roi_align_fwd");
}

int hvr_roi_align_bwd(const float* grad_out, const float* rois, float* grad_feat, int B, int C, int H, int W, int K, int PH,
                      int PW, float spatial_scale, int sample_num, int layout, void* stream) {
  (void)B;
  if (K == 0) return HVR_OK;
  if (!grad_out || !rois || !grad_feat) return fail(HVR_EINVAL, "null pointer");
  return check_launch(run_roi_align_bwd(grad_out, rois, grad_feat, C, H, W, K, PH, PW, spatial_scale, sample_num, layout,
                                        (hipStream_t)stream),
                      "hvr_roi_align_bwd");
}

// ---- deformable im2col (dcn.hip) ----
int hvr_deform_im2col_supported(int Cin, int deformable_groups, int dtype) {
  if (!valid_dtype(dtype) || Cin <= 0 || deformable_groups <= 0) return 0;
  return Cin % kstep_elems(dtype) == 0 && Cin % deformable_groups == 0 && (Cin / deformable_groups) % 8 == 0;
}

int hvr_deform_im2col(const void* x, const float* om, void* col, int B, int H, int W, int Cin, int KH, int KW, int stride, int pad, int dil,
                      int deformable_groups, int modulated, int64_t ldo, int dtype, void* stream) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "hvr_deform_im2col: bad dtype %d", dtype);
  if (!x || !om || !col) return fail(HVR_EINVAL, "hvr_deform_im2col: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0 || dil <= 0 || deformable_groups <= 0)
    return fail(HVR_EINVAL, "hvr_deform_im2col: bad shape B=%d H=%d W=%d Cin=%d k=%dx%d stride=%d pad=%d dil=%d groups=%d", B, H, W, Cin, KH, KW,
                stride, pad, dil, deformable_groups);
  if (Cin % kstep_elems(dtype)) return fail(HVR_EINVAL, "hvr_deform_im2col: Cin=%d is not a multiple of the %d-element K-step", Cin, kstep_elems(dtype));
  if (Cin % deformable_groups || (Cin / deformable_groups) % 8)
    return fail(HVR_EINVAL, "hvr_deform_im2col: Cin=%d over %d deformable groups is not a multiple of 8 channels per group", Cin, deformable_groups);
  const long OH = ((long)H + 2L * pad - (long)dil * (KH - 1) - 1) / stride + 1, OW = ((long)W + 2L * pad - (long)dil * (KW - 1) - 1) / stride + 1;
  if ((long)H + 2L * pad - (long)dil * (KH - 1) - 1 < 0 || (long)W + 2L * pad - (long)dil * (KW - 1) - 1 < 0)
    return fail(HVR_EINVAL, "hvr_deform_im2col: empty output");
  const long need = (long)(modulated ? 3 : 2) * deformable_groups * KH * KW;
  if (ldo < need) return fail(HVR_EINVAL, "hvr_deform_im2col: ldo=%ld is below the %ld offset%s channels", (long)ldo, need, modulated ? " + mask" : "");
  if (dtype == HVR_F16S ? (!aligned128(x) || !aligned128(col)) : (!aligned16(x) || !aligned16(col)))
    return fail(HVR_EINVAL, "hvr_deform_im2col: x and col must be 16-byte (split half: 128-byte) aligned");
  if ((reinterpret_cast<uintptr_t>(om) & 3) != 0) return fail(HVR_EINVAL, "hvr_deform_im2col: om must be 4-byte aligned");
  const long M = (long)B * OH * OW;
  if (M > 0x7fffffffL || (long)KH * KW > 4096) return fail(HVR_EUNSUPPORTED, "hvr_deform_im2col: too many output pixels or taps");
  return check_launch(run_deform_im2col(x, om, col, B, H, W, Cin, (int)OH, (int)OW, KH, KW, stride, pad, dil, deformable_groups, (long)ldo,
                                        modulated != 0, dtype, (hipStream_t)stream),
                      "hvr_deform_im2col");
}

// ---- deformable RoI pooling (dpool.hip) ----
int hvr_deform_roi_pool_fwd(const void* feat, const float* rois, const float* trans, const float* mask_logit, void* out, int B, int H, int W, int C,
                            int K, int PH, int PW, int out_channels, int group_size, int part_size, int num_classes, int sample_per_part,
                            float spatial_scale, float trans_std, int64_t ldt, int64_t ldm, int dtype, void* stream) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: bad dtype %d", dtype);
  if (dtype == HVR_F16S) return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: no split-half instance (pool in f32 and convert)");
  if (PH != PW) return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: out_size %d x %d is not square", PH, PW);
  if (K < 0 || B <= 0 || H <= 0 || W <= 0 || C <= 0 || PH <= 0 || out_channels <= 0 || group_size <= 0 || part_size <= 0 || num_classes <= 0 ||
      sample_per_part <= 0)
    return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: bad shape K=%d B=%d H=%d W=%d C=%d out_size=%d out_channels=%d group_size=%d part_size=%d classes=%d "
                "sample_per_part=%d", K, B, H, W, C, PH, out_channels, group_size, part_size, num_classes, sample_per_part);
  if ((long)C != (long)out_channels * group_size * group_size)
    return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: C=%d is not out_channels * group_size^2 = %d * %d^2", C, out_channels, group_size);
  if (out_channels % num_classes)
    return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: out_channels=%d is not a multiple of the %d offset classes", out_channels, num_classes);
  if (!(trans_std >= 0.f && trans_std <= 1.f)) return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: trans_std=%g is outside [0, 1]", (double)trans_std);
  if (PH > 1024 || part_size > 1024 || sample_per_part > 1024 || (long)H * W >= (1L << 31))
    return fail(HVR_EUNSUPPORTED, "hvr_deform_roi_pool_fwd: out_size, part_size, sample_per_part above 1024 or a map of 2^31 pixels");
  if (K == 0) return HVR_OK;
  if (!feat || !rois || !out) return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: null pointer");
  if (trans && ldt < (long)num_classes * 2 * part_size * part_size)
    return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: ldt=%ld is below the %ld offsets of a RoI", (long)ldt, (long)num_classes * 2 * part_size * part_size);
  if (!trans && num_classes != 1) return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: %d offset classes without offsets", num_classes);
  if (mask_logit && ldm < (long)PH * PW) return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: ldm=%ld is below the %d mask logits of a RoI", (long)ldm, PH * PW);
  const uintptr_t es = (uintptr_t)elem_size(dtype) - 1;
  if ((reinterpret_cast<uintptr_t>(feat) & es) || (reinterpret_cast<uintptr_t>(out) & es) || (reinterpret_cast<uintptr_t>(rois) & 3) ||
      (reinterpret_cast<uintptr_t>(trans) & 3) || (reinterpret_cast<uintptr_t>(mask_logit) & 3))
    return fail(HVR_EINVAL, "hvr_deform_roi_pool_fwd: misaligned pointer");
  return check_launch(run_deform_roi_pool(feat, rois, trans, mask_logit, out, B, H, W, C, K, PH, out_channels, group_size, part_size, num_classes,
                                          sample_per_part, spatial_scale, trans_std, (long)ldt, (long)ldm, dtype, (hipStream_t)stream),
                      "hvr_deform_roi_pool_fwd");
}

// ---- RoI max pooling (roi_pool.hip) ----
static int roi_pool_shape(const char* what, int B, int H, int W, int C, int K, int PH, int PW) {
  if (K < 0 || B < 0 || H <= 0 || W <= 0 || C <= 0 || PH <= 0 || PW <= 0)
    return fail(HVR_EINVAL, "%s: bad shape K=%d B=%d H=%d W=%d C=%d out_size=%d x %d", what, K, B, H, W, C, PH, PW);
  if ((long)H * W >= (1L << 31) || (long)PH * PW >= (1L << 31))
    return fail(HVR_EUNSUPPORTED, "%s: a map or an output of 2^31 cells (the argmax is an int32 within the frame's plane)", what);
  return HVR_OK;
}

int hvr_roi_pool_fwd(const void* feat, const float* rois, void* out, int32_t* argmax, int B, int H, int W, int C, int K, int PH, int PW,
                     float spatial_scale, int dtype, void* stream) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "hvr_roi_pool_fwd: bad dtype %d", dtype);
  if (dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "hvr_roi_pool_fwd: no split-half instance (pool in f32 and convert)");
  if (const int rc = roi_pool_shape("hvr_roi_pool_fwd", B, H, W, C, K, PH, PW)) return rc;
  const int cv = 16 / elem_size(dtype);
  if (C % cv) return fail(HVR_EUNSUPPORTED, "hvr_roi_pool_fwd: C=%d is not a multiple of %d (16 bytes of channels per lane)", C, cv);
  if (K == 0) return HVR_OK;
  if (!feat || !rois || !out) return fail(HVR_EINVAL, "hvr_roi_pool_fwd: null pointer");
  if (!aligned16(feat) || !aligned16(out) || !aligned16(argmax) || (reinterpret_cast<uintptr_t>(rois) & 3))
    return fail(HVR_EINVAL, "hvr_roi_pool_fwd: feat, out and argmax must be 16-byte aligned, rois 4-byte");
  return check_launch(run_roi_pool_fwd(feat, rois, out, argmax, B, H, W, C, K, PH, PW, spatial_scale, dtype, (hipStream_t)stream), "hvr_roi_pool_fwd");
}

int hvr_roi_pool_bwd(const float* grad_out, const float* rois, const int32_t* argmax, float* grad_feat, int B, int H, int W, int C, int K, int PH,
                     int PW, void* stream) {
  if (const int rc = roi_pool_shape("hvr_roi_pool_bwd", B, H, W, C, K, PH, PW)) return rc;
  if (K == 0) return HVR_OK;
  if (!grad_out || !rois || !argmax || !grad_feat) return fail(HVR_EINVAL, "hvr_roi_pool_bwd: null pointer");
  if ((reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(rois) | reinterpret_cast<uintptr_t>(argmax) |
       reinterpret_cast<uintptr_t>(grad_feat)) & 3)
    return fail(HVR_EINVAL, "hvr_roi_pool_bwd: misaligned pointer");
  return check_launch(run_roi_pool_bwd(grad_out, rois, argmax, grad_feat, B, H, W, C, K, PH, PW, (hipStream_t)stream), "hvr_roi_pool_bwd");
}

// ---- FPN top-down merge and multi-level RoIAlign (fpn.hip) ----
static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

int hvr_fpn_merge_supported(int L, int C, int dtype) {
  if (L < 1 || L > HVR_FPN_MAX_LEVELS || C <= 0 || C > 65536) return 0;
  if (dtype == HVR_F32) return C % 4 == 0;
  if (dtype == HVR_BF16 || dtype == HVR_F16) return C % 8 == 0;
  return 0;
}

int hvr_fpn_merge(const void* const* lat, void* const* out, int L, int B, const int32_t* H, const int32_t* W, int C, int dtype, void* stream) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "hvr_fpn_merge: bad dtype %d", dtype);
  if (L < 1 || B < 0 || C <= 0 || !H || !W || !lat) return fail(HVR_EINVAL, "hvr_fpn_merge: bad shape L=%d B=%d C=%d or a null array", L, B, C);
  if (!hvr_fpn_merge_supported(L, C, dtype))
    return fail(HVR_EUNSUPPORTED, "hvr_fpn_merge: no instance for L=%d C=%d dtype=%d (1 <= L <= %d; C a multiple of 16 bytes of channels, "
                "at most 65536; f32, bf16 or half)", L, C, dtype, HVR_FPN_MAX_LEVELS);
  if (L > 1 && !out) return fail(HVR_EINVAL, "hvr_fpn_merge: null output array");
  for (int l = 0; l < L; ++l) {
    if (H[l] <= 0 || W[l] <= 0) return fail(HVR_EINVAL, "hvr_fpn_merge: level %d is %d x %d", l, H[l], W[l]);
    if (l + 1 < L && (H[l] != 2 * H[l + 1] || W[l] != 2 * W[l + 1]))
      return fail(HVR_EINVAL, "hvr_fpn_merge: size mismatch, level %d is %d x %d and level %d is %d x %d (each level is exactly twice the next)",
                  l, H[l], W[l], l + 1, H[l + 1], W[l + 1]);
    if ((long)B * H[l] * W[l] >= (1L << 31)) return fail(HVR_EUNSUPPORTED, "hvr_fpn_merge: level %d has 2^31 pixels or more", l);
  }
  if (B == 0 || L == 1) return HVR_OK;
  const size_t es = (size_t)elem_size(dtype);
  size_t bytes[HVR_FPN_MAX_LEVELS];
  for (int l = 0; l < L; ++l) {
    bytes[l] = (size_t)B * H[l] * W[l] * C * es;
    if (!lat[l] || !aligned16(lat[l])) return fail(HVR_EINVAL, "hvr_fpn_merge: lat[%d] is null or not 16-byte aligned", l);
    if (l < L - 1 && (!out[l] || !aligned16(out[l]))) return fail(HVR_EINVAL, "hvr_fpn_merge: out[%d] is null or not 16-byte aligned", l);
  }
  for (int l = 0; l < L - 1; ++l) {
    for (int j = 0; j < L; ++j)
      if (ranges_overlap(out[l], bytes[l], lat[j], bytes[j])) return fail(HVR_EINVAL, "hvr_fpn_merge: out[%d] aliases lat[%d]", l, j);
    for (int j = l + 1; j < L - 1; ++j)
      if (ranges_overlap(out[l], bytes[l], out[j], bytes[j])) return fail(HVR_EINVAL, "hvr_fpn_merge: out[%d] aliases out[%d]", l, j);
  }
  return check_launch(run_fpn_merge(lat, out, L, B, H, W, C, dtype, (hipStream_t)stream), "hvr_fpn_merge");
}

int hvr_roi_align_levels_supported(int L, int C, int dtype) {
  return L >= 1 && L <= HVR_FPN_MAX_LEVELS && C > 0 && roi_align_levels_instance(C, dtype);
}

int hvr_roi_align_levels_fwd(const hvr_roi_levels_desc* d, void* stream) {
  if (!d) return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: null descriptor");
  if (!valid_dtype(d->dtype)) return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: bad dtype %d", d->dtype);
  if (d->dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "hvr_roi_align_levels_fwd: no split-half instance (pool in f32 and convert)");
  if (d->L < 1 || d->L > HVR_FPN_MAX_LEVELS) return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: L=%d is outside 1 .. %d", d->L, HVR_FPN_MAX_LEVELS);
  if (d->K < 0 || d->B <= 0 || d->C <= 0 || d->PH <= 0 || d->PW <= 0 || d->sample_num < 0)
    return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: bad shape K=%d B=%d C=%d out_size=%d x %d sample_num=%d", d->K, d->B, d->C, d->PH, d->PW,
                d->sample_num);
  if (!(d->finest_scale > 0.f)) return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: finest_scale=%g is not positive", (double)d->finest_scale);
  for (int l = 0; l < d->L; ++l)
    if (d->H[l] <= 0 || d->W[l] <= 0 || (long)d->H[l] * d->W[l] >= (1L << 31))
      return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: level %d is %d x %d", l, d->H[l], d->W[l]);
  if (!roi_align_levels_instance(d->C, d->dtype))
    return fail(HVR_EUNSUPPORTED, "hvr_roi_align_levels_fwd: no instance for C=%d dtype=%d (C a multiple of 4, at most 1024)", d->C, d->dtype);
  if (d->K == 0) return HVR_OK;
  if (!d->rois || !d->pool_rois || !d->out) return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: null pointer");
  const int al = d->dtype == HVR_F32 ? 15 : 7;   // what the widest load of the body needs when the 16-byte form is not taken
  for (int l = 0; l < d->L; ++l)
    if (!d->feat[l] || (reinterpret_cast<uintptr_t>(d->feat[l]) & al))
      return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: feat[%d] is null or misaligned", l);
  if ((reinterpret_cast<uintptr_t>(d->out) & al) || ((reinterpret_cast<uintptr_t>(d->rois) | reinterpret_cast<uintptr_t>(d->pool_rois) |
                                                      reinterpret_cast<uintptr_t>(d->levels)) & 3))
    return fail(HVR_EINVAL, "hvr_roi_align_levels_fwd: misaligned pointer");
  return check_launch(run_roi_align_levels(d->feat, d->H, d->W, d->spatial_scale, d->L, d->C, d->K, d->PH, d->PW, d->sample_num, d->dtype,
                                           d->finest_scale, d->rois, d->pool_rois, d->out, d->levels, (hipStream_t)stream),
                      "hvr_roi_align_levels_fwd");
}

// ---- NMS ----
size_t hvr_nms_workspace_bytes(int n) { return nms_ws(nullptr, 1, n).bytes + 256; }

int hvr_nms(const float* dets, int n, float thr, int ge_semantics, int64_t* keep, int32_t* n_keep, void* ws,
            size_t ws_bytes, void* stream) {
  if (!n_keep) return fail(HVR_EINVAL, "null n_keep");
  if (n == 0) {
    (void)run_zero_fill(n_keep, sizeof(int32_t), (hipStream_t)stream);
    return HVR_OK;
  }
  if (!dets || !keep || !ws) return fail(HVR_EINVAL, "null pointer");
  if (n < 0 || n > 8192) return fail(HVR_EUNSUPPORTED, "hvr_nms supports 0 <= n <= 8192, got %d", n);
  if (ws_bytes < hvr_nms_workspace_bytes(n)) return fail(HVR_EWORKSPACE, "nms workspace too small");
  return check_launch(run_nms_batched(dets, 1, n, thr, ge_semantics, 0, 0, (long long*)keep, n_keep, nms_ws(ws, 1, n), (hipStream_t)stream),
                      "hvr_nms");
}

int hvr_nms_first(const float* dets, int n, float thr, int ge_semantics, int max_keep, int64_t* keep, int32_t* n_keep, void* ws,
                  size_t ws_bytes, void* stream) {
  if (max_keep <= 0) return fail(HVR_EINVAL, "hvr_nms_first needs max_keep > 0 (hvr_nms keeps every survivor)");
  if (!n_keep) return fail(HVR_EINVAL, "null n_keep");
  if (n == 0) {
    (void)run_zero_fill(n_keep, sizeof(int32_t), (hipStream_t)stream);
    return HVR_OK;
  }
  if (!dets || !keep || !ws) return fail(HVR_EINVAL, "null pointer");
  if (n < 0 || n > 8192) return fail(HVR_EUNSUPPORTED, "hvr_nms_first supports 0 <= n <= 8192, got %d", n);
  if (ws_bytes < hvr_nms_workspace_bytes(n)) return fail(HVR_EWORKSPACE, "nms workspace too small");
  return check_launch(run_nms_batched(dets, 1, n, thr, ge_semantics, 0, max_keep, (long long*)keep, n_keep, nms_ws(ws, 1, n), (hipStream_t)stream),
                      "hvr_nms_first");
}

// ---- RPN ----
static inline int rpn_npre(int H, int W, int A, int nms_pre) {
  const long n = (long)H * W * A;
  return (nms_pre > 0 && n > nms_pre) ? nms_pre : (int)n;
}

// props [T][npre][5], keep [T][npre], n_keep [T], the NMS's buffers, the chip-wide select's (few frames)
struct RpnWs { float* props; long long* keep; int* n_keep; NmsWs nms; RpnWideWs wide; size_t bytes; };
static RpnWs rpn_ws(void* base, int T, int npre, long n_anchor) {
  Carver c(base);
  RpnWs L;
  L.props = c.take<float>((size_t)T * npre * 5);
  L.keep = c.take<long long>((size_t)T * npre);
  L.n_keep = c.take<int>((size_t)T);
  L.nms = nms_ws(c.here(), T, npre);
  c.skip(L.nms.bytes);
  L.wide = rpn_wide_ws(c.here(), T, n_anchor);
  c.skip(L.wide.bytes + 256);
  L.bytes = c.off;
  return L;
}

size_t hvr_rpn_workspace_bytes(int T, int H, int W, int A, int nms_pre) {
  return rpn_ws(nullptr, T, rpn_npre(H, W, A, nms_pre), (long)H * W * A).bytes;
}

int hvr_rpn_wide_frames(int frames) { return rpn_wide_max_frames(frames); }

int hvr_rpn_proposals(const hvr_rpn_desc* d, void* ws, size_t ws_bytes, void* stream) {
  if (!d || !ws) return fail(HVR_EINVAL, "null pointer");
  if (d->T <= 0) return fail(HVR_EINVAL, "hvr_rpn_proposals needs T >= 1 frames, got %d", d->T);
  if (d->A <= 0) return fail(HVR_EINVAL, "hvr_rpn_proposals needs A >= 1 base anchors, got %d", d->A);
  if (d->nms_post <= 0) return fail(HVR_EINVAL, "hvr_rpn_proposals needs nms_post > 0");
  if (d->max_num <= 0) return fail(HVR_EINVAL, "hvr_rpn_proposals needs max_num > 0");
  if (d->A > 32) return fail(HVR_EUNSUPPORTED, "at most 32 base anchors");
  const long n_anchor = (long)d->H * d->W * d->A;
  const int npre = rpn_npre(d->H, d->W, d->A, d->nms_pre);
  if (npre > 8192) return fail(HVR_EUNSUPPORTED, "nms_pre (or anchor count) above 8192");
  if (d->nms_post > 4096) return fail(HVR_EUNSUPPORTED, "nms_post above 4096");
  if (ws_bytes < hvr_rpn_workspace_bytes(d->T, d->H, d->W, d->A, d->nms_pre)) return fail(HVR_EWORKSPACE, "rpn workspace too small");
  RpnParams rp;
  rp.T = d->T; rp.H = d->H; rp.W = d->W; rp.A = d->A; rp.npre = npre; rp.n_anchor = (int)n_anchor;
  rp.cls_pitch = d->cls_pitch > 0 ? d->cls_pitch : d->A;
  rp.reg_pitch = d->reg_pitch > 0 ? d->reg_pitch : 4 * d->A;
  if (rp.cls_pitch < d->A || rp.reg_pitch < 4 * d->A || (rp.reg_pitch & 3)) return fail(HVR_EINVAL, "bad rpn pixel pitch");
  rp.stride = d->anchor_stride; rp.img_h = d->img_h; rp.img_w = d->img_w;
  for (int i = 0; i < 4; ++i) { rp.m[i] = d->means[i]; rp.s[i] = d->stds[i]; }
  rp.max_ratio = std::fabs(std::log(d->wh_ratio_clip));
  for (int a = 0; a < d->A; ++a)
    for (int i = 0; i < 4; ++i) rp.base[a][i] = d->base_anchors[a * 4 + i];
  const RpnWs L = rpn_ws(ws, d->T, npre, n_anchor);
  hipStream_t s = (hipStream_t)stream;
  const int presorted = n_anchor > npre ? 1 : 0;
  // few frames (stream mode: one): the chip-wide kernels -- the same proposals, bit for bit (nms.hip, "the chip-wide form")
  const bool wide = presorted && d->T <= rpn_wide_max_frames(-1) && d->nms_post > 0 && d->nms_post <= 1024;
  int rc;
  if (wide)
    rc = check_launch(run_rpn_select_wide(d->cls, d->reg, (long)d->H * d->W * rp.cls_pitch, (long)d->H * d->W * rp.reg_pitch, L.props, rp, L.wide, s), "rpn: select (chip-wide)");
  else
    rc = check_launch(run_rpn_select(d->cls, d->reg, (long)d->H * d->W * rp.cls_pitch, (long)d->H * d->W * rp.reg_pitch, L.props, rp, HVR_F32, s), "rpn: select");
  if (rc) return rc;
  // with score-sorted input the first nms_post survivors are known after nms_post keeps
  rc = check_launch(run_nms_batched(L.props, d->T, npre, d->nms_thr, 1, presorted, presorted ? d->nms_post : 0, L.keep, L.n_keep, L.nms, s,
                                    wide ? 4096 : 0, wide ? L.wide.done : nullptr),
                    "rpn: nms");
  if (rc) return rc;
  return check_launch(run_rpn_gather(L.props, L.keep, L.n_keep, d->T, npre, d->nms_post, d->max_num, presorted, d->proposals, d->counts, s),
                      "rpn: gather");
}

// ---- Guided Anchoring RPN (ga_rpn.hip) ----
int hvr_ga_mask_offsets(const float* loc, int64_t loc_pitch, float loc_filter_thr, uint8_t* keep, const float* shape, int64_t shape_pitch,
                        const float* w_off, float* om, int64_t ldo, int nch, int64_t pixels, void* stream) {
  if (!keep && !om) return fail(HVR_EINVAL, "hvr_ga_mask_offsets: neither a mask nor an offset output");
  if (pixels <= 0) return fail(HVR_EINVAL, "hvr_ga_mask_offsets: %ld pixels", (long)pixels);
  if (keep && (!loc || loc_pitch < 1)) return fail(HVR_EINVAL, "hvr_ga_mask_offsets: the mask needs loc and loc_pitch >= 1");
  if (om && (!shape || !w_off || shape_pitch < 2 || nch <= 0 || ldo < nch))
    return fail(HVR_EINVAL, "hvr_ga_mask_offsets: the offsets need shape (pitch >= 2), w_off, nch=%d >= 1 and ldo=%ld >= nch", nch, (long)ldo);
  if ((reinterpret_cast<uintptr_t>(loc) & 3) || (reinterpret_cast<uintptr_t>(shape) & 3) || (reinterpret_cast<uintptr_t>(w_off) & 3) ||
      (reinterpret_cast<uintptr_t>(om) & 3))
    return fail(HVR_EINVAL, "hvr_ga_mask_offsets: misaligned pointer");
  if (pixels > (1L << 40) / (om ? nch : 1)) return fail(HVR_EUNSUPPORTED, "hvr_ga_mask_offsets: too many outputs");
  return check_launch(run_ga_mask_offsets(loc, (long)loc_pitch, loc_filter_thr, keep, shape, (long)shape_pitch, w_off, om, (long)ldo, om ? nch : 1,
                                          (long)pixels, (hipStream_t)stream),
                      "hvr_ga_mask_offsets");
}

int hvr_masked_conv_max_cout(void) { return masked_conv_max_cout(); }

int hvr_masked_conv_fwd(const void* x, const void* w, const float* bias, const uint8_t* keep, float* out, int B, int H, int W, int Cin, int Cout,
                        int KH, int KW, int pad, int64_t ldo, int dtype, void* stream) {
  if (!valid_dtype(dtype)) return fail(HVR_EINVAL, "hvr_masked_conv_fwd: bad dtype %d", dtype);
  if (dtype == HVR_F16S) return fail(HVR_EUNSUPPORTED, "hvr_masked_conv_fwd: no split-half instance (run the f32 form)");
  if (!x || !w || !keep || !out) return fail(HVR_EINVAL, "hvr_masked_conv_fwd: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0)
    return fail(HVR_EINVAL, "hvr_masked_conv_fwd: bad shape B=%d H=%d W=%d Cin=%d Cout=%d k=%dx%d", B, H, W, Cin, Cout, KH, KW);
  if (KH != KW || (KH & 1) == 0 || pad != (KH - 1) / 2)
    return fail(HVR_EINVAL, "hvr_masked_conv_fwd: kernel %dx%d pad %d is not odd, square and padded to the input size", KH, KW, pad);
  if (Cin % (dtype == HVR_F32 ? 4 : 8)) return fail(HVR_EINVAL, "hvr_masked_conv_fwd: Cin=%d is not a whole number of 16-byte chunks", Cin);
  if (ldo < Cout) return fail(HVR_EINVAL, "hvr_masked_conv_fwd: ldo=%ld is below Cout=%d", (long)ldo, Cout);
  if (!aligned16(x) || !aligned16(w) || (reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(bias) & 3))
    return fail(HVR_EINVAL, "hvr_masked_conv_fwd: x and w must be 16-byte, out and bias 4-byte aligned");
  if (Cout > masked_conv_max_cout())
    return fail(HVR_EUNSUPPORTED, "hvr_masked_conv_fwd: Cout=%d is above the %d outputs of the skinny kernel (run the dense conv and zero the unkept pixels)",
                Cout, masked_conv_max_cout());
  if (KH > 15 || (long)B * H * W > 0x7fffffffL) return fail(HVR_EUNSUPPORTED, "hvr_masked_conv_fwd: kernel above 15x15 or 2^31 pixels");
  return check_launch(run_masked_conv(x, w, bias, keep, out, B, H, W, Cin, Cout, KH, pad, (long)ldo, dtype, (hipStream_t)stream), "hvr_masked_conv_fwd");
}

static inline int ga_npre(int H, int W, int nms_pre) {
  const long n = (long)H * W;
  return (nms_pre > 0 && n > nms_pre) ? nms_pre : (int)n;
}

// props [T][npre][5], keep [T][npre], n_keep / ncand / topk [T] each, pix [T][npre], the NMS's buffers
struct GaRpnWs { float* props; long long* keep; int *n_keep, *ncand, *topk, *pix; NmsWs nms; size_t bytes; };
static GaRpnWs ga_rpn_ws(void* base, int T, int npre) {
  Carver c(base);
  GaRpnWs L;
  L.props = c.take<float>((size_t)T * npre * 5);
  L.keep = c.take<long long>((size_t)T * npre);
  L.n_keep = c.take<int>((size_t)T);
  L.ncand = c.take<int>((size_t)T);
  L.topk = c.take<int>((size_t)T);
  L.pix = c.take<int>((size_t)T * npre);
  L.nms = nms_ws(c.here(), T, npre);
  c.skip(L.nms.bytes + 256);
  L.bytes = c.off;
  return L;
}

size_t hvr_ga_rpn_workspace_bytes(int T, int H, int W, int nms_pre) {
  if (T <= 0 || H <= 0 || W <= 0 || (long)H * W > 8192) return 0;
  return ga_rpn_ws(nullptr, T, ga_npre(H, W, nms_pre)).bytes;
}

int hvr_ga_rpn_proposals(const hvr_ga_rpn_desc* d, void* ws, size_t ws_bytes, void* stream) {
  if (!d || !ws) return fail(HVR_EINVAL, "hvr_ga_rpn_proposals: null pointer");
  if (d->T <= 0 || d->H <= 0 || d->W <= 0) return fail(HVR_EINVAL, "hvr_ga_rpn_proposals needs T, H, W >= 1, got %d, %d, %d", d->T, d->H, d->W);
  if (d->nms_post <= 0) return fail(HVR_EINVAL, "hvr_ga_rpn_proposals needs nms_post > 0");
  if (d->max_num <= 0) return fail(HVR_EINVAL, "hvr_ga_rpn_proposals needs max_num > 0");
  if (!d->cls || !d->reg || !d->shape || !d->keep || !d->proposals || !d->counts || !d->base_square || !d->anchoring_means ||
      !d->anchoring_stds || !d->target_means || !d->target_stds)
    return fail(HVR_EINVAL, "hvr_ga_rpn_proposals: null pointer in the descriptor");
  if ((long)d->H * d->W > 8192) return fail(HVR_EUNSUPPORTED, "hvr_ga_rpn_proposals: a map of %d x %d is above 8192 pixels", d->H, d->W);
  if (d->nms_post > 4096) return fail(HVR_EUNSUPPORTED, "hvr_ga_rpn_proposals: nms_post above 4096");
  if (!(d->wh_ratio_clip > 0.f) || !std::isfinite(d->wh_ratio_clip))
    return fail(HVR_EINVAL, "hvr_ga_rpn_proposals needs a finite wh_ratio_clip > 0, got %g", (double)d->wh_ratio_clip);
  GaParams gp;
  gp.T = d->T; gp.H = d->H; gp.W = d->W; gp.nms_pre = d->nms_pre; gp.stride = d->anchor_stride;
  gp.npre = ga_npre(d->H, d->W, d->nms_pre);
  gp.cls_pitch = d->cls_pitch > 0 ? d->cls_pitch : 1;
  gp.reg_pitch = d->reg_pitch > 0 ? d->reg_pitch : 4;
  gp.shape_pitch = d->shape_pitch > 0 ? d->shape_pitch : 2;
  if (gp.reg_pitch < 4 || gp.shape_pitch < 2) return fail(HVR_EINVAL, "hvr_ga_rpn_proposals: bad pixel pitch");
  if ((reinterpret_cast<uintptr_t>(d->cls) & 3) || (reinterpret_cast<uintptr_t>(d->reg) & 3) || (reinterpret_cast<uintptr_t>(d->shape) & 3))
    return fail(HVR_EINVAL, "hvr_ga_rpn_proposals: misaligned map");
  if (ws_bytes < hvr_ga_rpn_workspace_bytes(d->T, d->H, d->W, d->nms_pre)) return fail(HVR_EWORKSPACE, "ga rpn workspace too small");
  for (int i = 0; i < 4; ++i) {
    gp.square[i] = d->base_square[i];
    gp.am[i] = d->anchoring_means[i]; gp.as[i] = d->anchoring_stds[i];
    gp.tm[i] = d->target_means[i];    gp.ts[i] = d->target_stds[i];
  }
  gp.a_ratio = std::fabs(std::log(1e-6f));
  gp.t_ratio = std::fabs(std::log(d->wh_ratio_clip));
  gp.img_h = d->img_h; gp.img_w = d->img_w;
  const int npre = gp.npre;
  const GaRpnWs L = ga_rpn_ws(ws, d->T, npre);
  hipStream_t s = (hipStream_t)stream;
  int rc = check_launch(run_ga_select(d->cls, d->reg, d->shape, d->keep, L.props, L.pix, L.ncand, L.topk, gp, s), "ga rpn: select");
  if (rc) return rc;
  // Every survivor is needed: whether a frame's "first nms_post" are the first in score order (its top nms_pre were taken) or in
  // row-major order (they were not) depends on its kept count, which only the device knows -- no cap on the NMS.
  rc = check_launch(run_nms_batched(L.props, d->T, npre, d->nms_thr, 1, 1, 0, L.keep, L.n_keep, L.nms, s), "ga rpn: nms");
  if (rc) return rc;
  return check_launch(run_ga_gather(L.props, L.keep, L.n_keep, L.pix, L.ncand, L.topk, d->T, npre, d->nms_post, d->max_num, d->proposals, d->counts, s),
                      "ga rpn: gather");
}

// ---- RCNN read-out ----
int hvr_det_decode(const float* logits, int ldl, int cls_off, int reg_off, int ncls, const float* rois, int R,
                   const float* means, const float* stds, float wh_ratio_clip, float img_h, float img_w,
                   float scale_factor, float* scores, float* boxes, void* stream) {
  if (R == 0) return HVR_OK;
  if (!logits || !rois || !scores || !boxes || !means || !stds) return fail(HVR_EINVAL, "null pointer");
  return check_launch(run_det_decode(logits, ldl, cls_off, reg_off, ncls, rois, R, means, stds,
                                     std::fabs(std::log(wh_ratio_clip)), img_h, img_w, scale_factor, scores, boxes,
                                     (hipStream_t)stream),
                      "hvr_det_decode");
}

size_t hvr_multiclass_nms_workspace_bytes(int R, int ncls) { return multiclass_nms_workspace_bytes(R, ncls); }

int hvr_multiclass_nms(const float* boxes, const float* scores, int R, int ncls, float score_thr, float iou_thr, int max_num,
                       float* dets, int64_t* labels, int32_t* n_out, void* ws, size_t ws_bytes, void* stream) {
  if (!n_out) return fail(HVR_EINVAL, "null n_out");
  if (R == 0) {
    (void)run_zero_fill(n_out, sizeof(int32_t), (hipStream_t)stream);
    return HVR_OK;
  }
  if (R < 0 || R > 512) return fail(HVR_EUNSUPPORTED, "hvr_multiclass_nms supports R <= 512, got %d", R);
  if (ncls < 2 || ncls - 1 > 128) return fail(HVR_EUNSUPPORTED, "hvr_multiclass_nms supports 1 .. 128 foreground classes");
  if (max_num <= 0) return fail(HVR_EINVAL, "hvr_multiclass_nms needs max_num > 0");
  if ((long)(ncls - 1) * R > multiclass_nms_max_candidates())
    return fail(HVR_EUNSUPPORTED, "hvr_multiclass_nms supports (ncls - 1) * R <= %d candidates (the merge kernel's list in LDS), got %ld",
                multiclass_nms_max_candidates(), (long)(ncls - 1) * R);
  if (!boxes || !scores || !dets || !labels || !ws) return fail(HVR_EINVAL, "null pointer");
  if (ws_bytes < hvr_multiclass_nms_workspace_bytes(R, ncls)) return fail(HVR_EWORKSPACE, "multiclass nms workspace too small");
  return check_launch(run_multiclass_nms(boxes, scores, R, ncls, score_thr, iou_thr, max_num, dets, (long long*)labels, n_out,
                                         mc_nms_ws(ws, R, ncls), (hipStream_t)stream),
                      "hvr_multiclass_nms");
}

// ---- Soft-NMS read-out (softnms.hip) ----
size_t hvr_soft_nms_workspace_bytes(int n) { (void)n; return 256; }   // (the single list lives in LDS; kept for the calling convention)

int hvr_soft_nms(const float* dets, int n, float iou_thr, int method, float sigma, float min_score, float* out_dets, int64_t* inds,
                 int32_t* n_out, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  if (!n_out) return fail(HVR_EINVAL, "null n_out");
  if (method != 1 && method != 2) return fail(HVR_EINVAL, "hvr_soft_nms: method is 1 (linear) or 2 (gaussian), got %d", method);
  if (n == 0) {
    (void)run_zero_fill(n_out, sizeof(int32_t), (hipStream_t)stream);
    return HVR_OK;
  }
  if (!dets || !out_dets || !inds) return fail(HVR_EINVAL, "null pointer");
  if (n < 0 || n > 512) return fail(HVR_EUNSUPPORTED, "hvr_soft_nms supports 0 <= n <= 512, got %d", n);
  if (ws_bytes < hvr_soft_nms_workspace_bytes(n)) return fail(HVR_EWORKSPACE, "soft nms workspace too small");
  return check_launch(run_soft_nms(dets, n, iou_thr, method, sigma, min_score, out_dets, (long long*)inds, n_out, (hipStream_t)stream),
                      "hvr_soft_nms");
}

size_t hvr_multiclass_soft_nms_workspace_bytes(int P, int R, int ncls) {
  return mc_soft_nms_ws(nullptr, P > 0 ? P : 1, R > 0 ? R : 1, ncls > 1 ? ncls : 2).bytes;
}

int hvr_multiclass_soft_nms(const float* boxes, const float* scores, int P, int R, int ncls, float score_thr, float iou_thr, int method,
                            float sigma, float min_score, int max_num, float* dets, int64_t* labels, int32_t* n_out, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!n_out) return fail(HVR_EINVAL, "null n_out");
  if (P < 1) return fail(HVR_EINVAL, "hvr_multiclass_soft_nms needs P >= 1 problems, got %d", P);
  if (method != 1 && method != 2) return fail(HVR_EINVAL, "hvr_multiclass_soft_nms: method is 1 (linear) or 2 (gaussian), got %d", method);
  if (R == 0) {
    (void)run_zero_fill(n_out, sizeof(int32_t) * (size_t)P, (hipStream_t)stream);
    return HVR_OK;
  }
  if (!boxes || !scores || !dets || !labels || !ws) return fail(HVR_EINVAL, "null pointer");
  if (R < 0 || R > 512) return fail(HVR_EUNSUPPORTED, "hvr_multiclass_soft_nms supports R <= 512, got %d", R);
  if (ncls < 2 || ncls - 1 > 128) return fail(HVR_EUNSUPPORTED, "hvr_multiclass_soft_nms supports 1 .. 128 foreground classes");
  if (max_num <= 0) return fail(HVR_EINVAL, "hvr_multiclass_soft_nms needs max_num > 0");
  if (ws_bytes < hvr_multiclass_soft_nms_workspace_bytes(P, R, ncls)) return fail(HVR_EWORKSPACE, "multiclass soft nms workspace too small");
  return check_launch(run_multiclass_soft_nms(boxes, scores, P, R, ncls, score_thr, iou_thr, method, sigma, min_score, max_num, dets,
                                              (long long*)labels, n_out, mc_soft_nms_ws(ws, P, R, ncls), (hipStream_t)stream),
                      "hvr_multiclass_soft_nms");
}

// ---- Seq-NMS read-out of a whole video (seqnms.hip) ----
size_t hvr_seq_nms_workspace_bytes(int F, int R, int ncls) {
  return seq_nms_ws(nullptr, 1, F > 0 ? F : 1, R > 0 ? R : 1, ncls > 1 ? ncls : 2, false).bytes;
}

size_t hvr_seq_nms_batched_workspace_bytes(int P, int Ftot, int R, int ncls, int tubes) {
  return seq_nms_ws(nullptr, P > 0 ? P : 1, Ftot > 0 ? Ftot : 1, R > 0 ? R : 1, ncls > 1 ? ncls : 2, tubes != 0).bytes;
}

int hvr_seq_nms(const float* boxes, const float* scores, int F, int R, int ncls, float score_thr, float link_thr, float nms_thr,
                int rescore, int max_num, float* dets, int64_t* labels, int32_t* n_out, void* ws, size_t ws_bytes, void* stream) {
  return hvr_seq_nms_phases(boxes, scores, F, R, ncls, score_thr, link_thr, nms_thr, rescore, max_num, dets, labels, n_out, ws, ws_bytes, 7,
                            stream);
}

int hvr_seq_nms_phases(const float* boxes, const float* scores, int F, int R, int ncls, float score_thr, float link_thr, float nms_thr,
                       int rescore, int max_num, float* dets, int64_t* labels, int32_t* n_out, void* ws, size_t ws_bytes, int phases,
                       void* stream) {
  if (phases < 1 || phases > 7) return fail(HVR_EINVAL, "hvr_seq_nms_phases: phases is a mask of 1 (link) | 2 (path) | 4 (merge), got %d", phases);
  if (!n_out) return fail(HVR_EINVAL, "null n_out");
  if (F < 1) return fail(HVR_EINVAL, "hvr_seq_nms needs F >= 1 frames, got %d", F);
  if (rescore != 1 && rescore != 2) return fail(HVR_EINVAL, "hvr_seq_nms: rescore is 1 (avg) or 2 (max), got %d", rescore);
  if (!(score_thr >= 0.f)) return fail(HVR_EINVAL, "hvr_seq_nms needs score_thr >= 0 (path sums must be positive), got %g", (double)score_thr);
  if (link_thr != link_thr || nms_thr != nms_thr) return fail(HVR_EINVAL, "hvr_seq_nms: NaN threshold");
  if (max_num <= 0) return fail(HVR_EINVAL, "hvr_seq_nms needs max_num > 0");
  if (R < 0 || R > 512) return fail(HVR_EUNSUPPORTED, "hvr_seq_nms supports R <= 512, got %d", R);
  if (F > 65535) return fail(HVR_EUNSUPPORTED, "hvr_seq_nms supports at most 65535 frames per video, got %d", F);
  if (ncls < 2 || ncls - 1 > 128) return fail(HVR_EUNSUPPORTED, "hvr_seq_nms supports 1 .. 128 foreground classes");
  if (R == 0) {
    (void)run_zero_fill(n_out, sizeof(int32_t) * (size_t)F, (hipStream_t)stream);
    return HVR_OK;
  }
  if (!boxes || !scores || !dets || !labels || !ws) return fail(HVR_EINVAL, "null pointer");
  if (!aligned16(boxes) || !aligned16(ws)) return fail(HVR_EINVAL, "hvr_seq_nms: boxes and workspace must be 16-byte aligned");
  if (ws_bytes < hvr_seq_nms_workspace_bytes(F, R, ncls)) return fail(HVR_EWORKSPACE, "seq nms workspace too small");
  return check_launch(run_seq_nms(boxes, scores, 1, nullptr, F, R, ncls, score_thr, link_thr, nms_thr, rescore == 2, max_num, dets,
                                  (long long*)labels, n_out, nullptr, nullptr, nullptr, nullptr, 0, seq_nms_ws(ws, 1, F, R, ncls, false), phases,
                                  (hipStream_t)stream),
                      "hvr_seq_nms");
}

// P problems side by side and, optionally, the tube outputs: the same three kernels (hvr_seq_nms is their P = 1, no-tubes case)
int hvr_seq_nms_batched(const float* boxes, const float* scores, int P, const int32_t* frame_start, int Ftot, int R, int ncls, float score_thr,
                        float link_thr, float nms_thr, int rescore, int max_num, float* dets, int64_t* labels, int32_t* n_out,
                        int32_t* tube_ids, int32_t* tubes, float* tube_scores, int32_t* tube_start, int max_tubes, void* ws, size_t ws_bytes,
                        void* stream) {
  const int want = (tube_ids != nullptr) + (tubes != nullptr) + (tube_scores != nullptr) + (tube_start != nullptr);
  if (want != 0 && want != 4) return fail(HVR_EINVAL, "hvr_seq_nms_batched: the four tube outputs are all NULL or all non-NULL");
  if (!n_out) return fail(HVR_EINVAL, "null n_out");
  if (P < 1) return fail(HVR_EINVAL, "hvr_seq_nms_batched needs P >= 1 problems, got %d", P);
  if (Ftot < P) return fail(HVR_EINVAL, "hvr_seq_nms_batched needs at least one frame per problem, got %d frames for %d problems", Ftot, P);
  if (rescore != 1 && rescore != 2) return fail(HVR_EINVAL, "hvr_seq_nms_batched: rescore is 1 (avg) or 2 (max), got %d", rescore);
  if (!(score_thr >= 0.f)) return fail(HVR_EINVAL, "hvr_seq_nms_batched needs score_thr >= 0 (path sums must be positive), got %g", (double)score_thr);
  if (link_thr != link_thr || nms_thr != nms_thr) return fail(HVR_EINVAL, "hvr_seq_nms_batched: NaN threshold");
  if (max_num <= 0) return fail(HVR_EINVAL, "hvr_seq_nms_batched needs max_num > 0");
  if (want && max_tubes < 0) return fail(HVR_EINVAL, "hvr_seq_nms_batched needs max_tubes >= 0, got %d", max_tubes);
  if (R < 0 || R > 512) return fail(HVR_EUNSUPPORTED, "hvr_seq_nms_batched supports R <= 512, got %d", R);
  if (Ftot > 65535) return fail(HVR_EUNSUPPORTED, "hvr_seq_nms_batched supports at most 65535 frames per call, got %d", Ftot);
  if (ncls < 2 || ncls - 1 > 128) return fail(HVR_EUNSUPPORTED, "hvr_seq_nms_batched supports 1 .. 128 foreground classes");
  if (R == 0) {   // only the counts: no box, no tube
    (void)run_zero_fill(n_out, sizeof(int32_t) * (size_t)Ftot, (hipStream_t)stream);
    if (want) (void)run_zero_fill(tube_start, sizeof(int32_t) * ((size_t)P + 1), (hipStream_t)stream);
    return HVR_OK;
  }
  if (!boxes || !scores || !frame_start || !dets || !labels || !ws) return fail(HVR_EINVAL, "null pointer");
  if (!aligned16(boxes) || !aligned16(ws) || (want && !aligned16(tubes)))
    return fail(HVR_EINVAL, "hvr_seq_nms_batched: boxes, workspace and the tube table must be 16-byte aligned");
  if (ws_bytes < hvr_seq_nms_batched_workspace_bytes(P, Ftot, R, ncls, want != 0)) return fail(HVR_EWORKSPACE, "seq nms workspace too small");
  return check_launch(run_seq_nms(boxes, scores, P, frame_start, Ftot, R, ncls, score_thr, link_thr, nms_thr, rescore == 2, max_num, dets,
                                  (long long*)labels, n_out, tube_ids, tubes, tube_scores, tube_start, max_tubes,
                                  seq_nms_ws(ws, P, Ftot, R, ncls, want != 0), 7, (hipStream_t)stream),
                      "hvr_seq_nms_batched");
}

// ---- plumbing ----
int hvr_cast(const void* in, void* out, int64_t n, int from_dtype, int to_dtype, void* stream) {
  return hvr_cast_scaled(in, out, n, from_dtype, to_dtype, 1.f, stream);
}

int hvr_cast_scaled(const void* in, void* out, int64_t n, int from_dtype, int to_dtype, float scale, void* stream) {
  if (n == 0) return HVR_OK;
  if (!in || !out) return fail(HVR_EINVAL, "null pointer");
  if (!valid_dtype(from_dtype) || !valid_dtype(to_dtype) || (from_dtype == to_dtype && (scale == 1.f || from_dtype != HVR_F32)))
    return fail(HVR_EINVAL, "bad cast %d -> %d", from_dtype, to_dtype);
  if (!(scale > 0.f)) return fail(HVR_EINVAL, "cast scale must be positive");
  const bool classic = scale == 1.f && ((from_dtype == HVR_F32 && to_dtype == HVR_BF16) || (from_dtype == HVR_BF16 && to_dtype == HVR_F32));
  if (!classic) {   // 8 elements per thread; split half moves whole 64-element groups
    const bool split = from_dtype == HVR_F16S || to_dtype == HVR_F16S;   // split half moves whole 32-element groups
    if (n % (split ? 32 : 8) || !aligned16(in) || !aligned16(out) || (from_dtype == HVR_F16S && !aligned128(in)) || (to_dtype == HVR_F16S && !aligned128(out)))
      return fail(HVR_EINVAL, "hvr_cast to / from half formats: n %% 8 == 0 (split half: n %% 32 == 0, 128-byte aligned), 16-byte aligned buffers");
  }
  return check_launch(run_cast(in, out, n, from_dtype, to_dtype, scale, (hipStream_t)stream), "hvr_cast");
}

int hvr_permute_nchw_nhwc(const void* in, void* out, int B, int C, int HW, int to_nhwc, int from_dtype, int to_dtype,
                          void* stream) {
  if (!in || !out || B <= 0 || C <= 0 || HW <= 0) return fail(HVR_EINVAL, "bad permute arguments");
  return check_launch(run_permute(in, out, B, C, HW, to_nhwc, from_dtype, to_dtype, (hipStream_t)stream), "hvr_permute");
}

int hvr_transpose_pad(const void* in, void* out, int R, int C, int64_t ldx, int64_t ldt, int dtype, void* stream) {
  if (!in || !out || R <= 0 || C <= 0 || ldt < R) return fail(HVR_EINVAL, "bad transpose arguments");
  return check_launch(run_transpose_pad(in, out, R, C, ldx, ldt, dtype, (hipStream_t)stream), "hvr_transpose_pad");
}

}  // extern "C"
