/*
 * hvr_hip -- C ABI of the MI355X (gfx950) kernels behind the HVRNet video-detection
 * forward path.  This is the drop-in boundary: every entry point below names the
 * reference interface it replaces (paths relative to the youthHan/HVRNet tree).
 *
 * Conventions (mirroring the reference's caller-allocates pybind ABI,
 * mmdet/ops/roi_align/src/roi_align_cuda.cpp:27-53, mmdet/ops/roi_align/roi_align.py:23):
 *   - every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *     the library never allocates, frees or retains memory;
 *   - work is enqueued on `stream` (hipStream_t passed as void*); nothing synchronises;
 *   - return 0 on success, a negative HVR_E* code otherwise; hvr_last_error() gives the
 *     message of the calling thread's last failure (the reference printf()s "wrong roi
 *     size" and carries on, roi_align_cuda.cpp:39-42 -- this library never does that);
 *   - dtype: HVR_F32 = 0, HVR_BF16 = 1, HVR_F16 = 2, HVR_F16S = 3 (element type of activations /
 *     weights; all accumulation, softmax, box and score arithmetic is f32) -- the precision ladder:
 *       HVR_BF16  bf16 operands, the benchmark dtype BASELINE.json names (v_mfma_f32_16x16x32_bf16);
 *       HVR_F16   IEEE half operands: the same rate and bytes, 8 x finer mantissa, range 65504;
 *       HVR_F16S  "split half": a logical element x is stored as hi = half(x), lo = half(x - hi) (22 significant
 *                 bits for |x| >= 2^-3, absolute error < 2^-24 below) and a product is three half MFMAs -- hi*hi + hi*lo +
 *                 lo*hi -- accumulated in f32: f32-grade results at 1/3 of the half MFMA rate.  Memory layout of a row
 *                 of C elements (C % 32 == 0): C / 32 groups of [32 hi halves][32 lo halves] = 4 bytes per logical
 *                 element, both planes of a 32-element K-step in one 128-byte line; leading dimensions stay in logical
 *                 elements, bases are 128-byte aligned, column offsets multiples of 32.  hvr_cast converts to and from it.  Taken by hvr_gemm, hvr_conv2d_nhwc, hvr_relation_fwd,
 *                 hvr_relation_probs, hvr_transpose_pad and hvr_cast; the other entry points return HVR_EUNSUPPORTED;
 *       HVR_F32   exact f32 (v_mfma_f32_16x16x4_f32, 1/16 of the half rate): the parity mode.
 *     The reference computes in f32 (no fp16 key in configs/faster_rcnn_r101_{selsa,hrnmp}_c5.py); its optional
 *     mixed-precision islands are mmdet/core/fp16/decorators.py:9-160.
 *   - re-entrant; the only global mutable state is the one-time per-device kernel attribute setup (atomic, idempotent) and ONE
 *     process-wide tuning knob, hvr_rpn_wide_frames (an atomic int: which of two bit-identical kernel forms hvr_rpn_proposals
 *     launches; a captured graph keeps the form chosen at capture time).
 *   - environment switches, read once per process (round 5 retired the tuning knobs of rounds 1-4: tile-shape hints, slice sizes,
 *     group sizes, thresholds and the variants that measured slower are gone).  What is left selects between kernels that compute
 *     the same thing, for A/B runs and for the tests that compare them:
 *       HVR_BIGTILE=0         no 288 x 256 tiles (csrc/bigtile.hip): the tile engine's shapes everywhere (bit-identical)
 *       HVR_EXPAND=0          no row-panel expand kernel (csrc/expand.hip): tile engine / big tiles
 *       HVR_CONV3=0           no weights-resident 3x3 kernel for Cin = 64 (csrc/conv3x3.hip): tile engine (bit-identical)
 *       HVR_CONV_SPLITK       few-row products given a workspace (stream mode's one-frame launches): 0 = unsplit; 1 (default) = K
 *                             sliced across the waves of a workgroup where the shape allows (csrc/kpar.hip: one launch, no
 *                             partials), else across workgroups + a reduce launch; 2 = always the latter
 *       HVR_SPLIT_NORMALIZE   split-half relation: 0 = block weights folded into the apply pass, 1 = one normalising sweep + plain
 *                             product (default: by query-row count)
 *       HVR_REL_GROUPED       hvr_relation_fwd_grouped: 0 = one hvr_relation_fwd per group, 1 = grouped scores + per-group apply,
 *                             2 (default) = + the grouped apply launch
 *       HVR_NMS_MASK          (set) hvr_nms always takes the bit-mask kernels, never the greedy small-cap kernel
 *       HVR_RPN_WIDE=<frames> initial value of hvr_rpn_wide_frames
 *     and, in the Python host layer, HVR_RPN_SIDE=0 (RPN branch on the caller's stream instead of a side stream).
 */
#ifndef HVR_HIP_H_
#define HVR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVR_OK 0
#define HVR_EINVAL (-1)       /* bad argument (shape, alignment, null pointer) */
#define HVR_EUNSUPPORTED (-2) /* valid request outside the implemented envelope */
#define HVR_ELAUNCH (-3)      /* HIP reported a launch error */
#define HVR_EWORKSPACE (-4)   /* workspace too small */

#define HVR_F32 0
#define HVR_BF16 1
#define HVR_F16 2
#define HVR_F16S 3

#define HVR_LAYOUT_NCHW 0 /* reference layout */
#define HVR_LAYOUT_NHWC 1 /* native layout of this library */

int hvr_abi_version(void);   /* 2 since the descriptors of hvr_gemm / hvr_conv2d_nhwc grew the split-K scratch fields; 3: HVR_F16 / HVR_F16S; 4: hvr_tail_next_desc carries alpha / beta (split-half operands); 5: hvr_relation_fwd_grouped; 6: hvr_gemm_splitk_batched / hvr_unpack_conv_wgrads_multi; 7: hvr_sample_pos_neg takes neg_pos_ub as a double */
const char* hvr_last_error(void);

/* ------------------------------------------------------------------------------------
 * Dense contraction with fused epilogue:  C[M][N] = act(A[M][K] . B[N][K]^T + bias + R)
 * Replaces the ATen calls behind nn.Linear / 1x1 Conv2d on the path:
 *   selsa_bbox_head.py:156,159,185-186,220-221,237 ; hrnmp_bbox_head.py:283,286,345-346,827-906.
 * K must be a multiple of 128 bytes / sizeof(elem); N a multiple of 4; rows 16-byte aligned.
 * staging: 0 = register-staged loads, 1 = direct global->LDS DMA.
 * ---------------------------------------------------------------------------------- */
typedef struct hvr_gemm_desc {
  const void* A; const void* B; void* C;
  int32_t M, N, K;
  int64_t lda, ldb, ldc;   /* in elements */
  const float* bias;       /* [N] f32 or NULL */
  const void* resid;       /* [M][ldr] (operand dtype) or NULL */
  int64_t ldr;
  int32_t relu;            /* apply max(x, 0) last */
  int32_t out_f32;         /* store C as f32 regardless of dtype */
  int32_t dtype;
  int32_t staging;
  int32_t tile_hint;       /* 0 = library picks the tile shape; k > 0 forces shape k-1 (tuning) */
  void* ws; size_t ws_bytes;   /* hvr_gemm: few-row split-K scratch (hvr_gemm_fewrow_workspace_bytes) or NULL / 0 */
  float alpha;             /* HVR_F16S only: C = act(alpha * (A . B^T) + bias + R), alpha a power of two (0 = 1).  A split-half
                              value below 2^-3 keeps an absolute, not a relative, error bound (its lo half is a subnormal), so
                              callers store small-magnitude operands scaled up -- this build's host layer keeps weights x 2^6 and
                              activations x 2^4 (hvr_cast_scaled) -- and pass the inverse here */
  float beta;              /* HVR_F16S only: factor on the bias (0 = 1): C = act(alpha * (A . B^T) + beta * bias + R) */
} hvr_gemm_desc;
/* Few-row products with an epilogue (one frame's 300 proposals through fc_new_1: 300 x 1024 x 12544 is 48 tiles of 128 x 64
 * walking 196 K-steps each): bytes of caller-owned scratch with which hvr_gemm cuts K into grid.y slices of f32 partial tiles
 * and applies bias / residual / ReLU in one reduce launch (bf16 operands and output).  0 = not split.  Without the scratch the
 * product runs unsplit (same result up to the f32 summation order).  The same rule as hvr_conv2d_splitk_workspace_bytes. */
size_t hvr_gemm_fewrow_workspace_bytes(const hvr_gemm_desc* d);
int hvr_gemm(const hvr_gemm_desc* d, void* stream);
/* The same product for outputs with few tiles and a long K (weight gradients: dW = dZ^T X has K = pixels): the K loop is cut
 * into slices that run as one launch, each writing an f32 partial into `ws`, and a second kernel sums them in a fixed order.
 * f32 output only (dtype f32, or out_f32 with bf16 operands), no bias / residual / ReLU.  The library picks the slice count
 * (1 = falls back to hvr_gemm's single pass; hvr_gemm_splitk_workspace_bytes then returns 0). */
size_t hvr_gemm_splitk_workspace_bytes(int M, int N, int K, int dtype);
int hvr_gemm_splitk(const hvr_gemm_desc* d, void* ws, size_t ws_bytes, void* stream);
/* `count` such products of ONE shape in one launch (round 6: the weight gradients of a ResNet stage's identical Bottlenecks -- the reference
 * differentiates each nn.Conv2d on its own, mmdet/models/backbones/resnet.py:220-266; at three frames per rank a single dW = dZ^T X leaves
 * most of the chip idle and costs three launches): d describes problem 0, problem g reads A + g * stride_a and B + g * stride_b ELEMENTS and
 * writes C + g * stride_c floats; f32 output, no epilogue.  The library cuts K into slices while count x tiles is below a round of the
 * chip; the sliced form needs the workspace below and one contiguous output (ldc = N, stride_c = M * N). */
size_t hvr_gemm_splitk_batched_workspace_bytes(int M, int N, int K, int dtype, int count);
int hvr_gemm_splitk_batched(const hvr_gemm_desc* d, int count, int64_t stride_a, int64_t stride_b, int64_t stride_c, void* ws, size_t ws_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * NHWC convolution as implicit GEMM (frozen BatchNorm folded into w / bias by the caller)
 * with fused bias + residual + ReLU.  Replaces nn.Conv2d + BatchNorm2d(eval) + ReLU (+ the
 * Bottleneck residual add): mmdet/models/backbones/resnet.py:220-266,
 * mmdet/models/shared_heads/res_layer.py:67-74, mmdet/models/anchor_heads/rpn_head.py:30-35.
 *   x [B][H][W][Cin], w [Cout][KH][KW][Cin], y [B][OH][OW][Cout]; Cin % (128/sizeof elem) == 0.
 *   zero: >= 16 readable zero bytes on the device (source of padding taps).
 * ---------------------------------------------------------------------------------- */
typedef struct hvr_conv_desc {
  const void* x; const void* w; void* y;
  int32_t B, H, W, Cin, Cout, KH, KW, stride, pad, dil;
  const float* bias;
  const void* resid;       /* [B][OH][OW][Cout] or NULL */
  int32_t relu, out_f32, dtype, staging, tile_hint;
  const void* zero;
  void* ws; size_t ws_bytes;   /* split-K workspace (see hvr_conv2d_splitk_workspace_bytes) or NULL / 0 */
  float alpha, beta;       /* HVR_F16S only: factors on the accumulators / the bias, see hvr_gemm_desc (0 = 1) */
} hvr_conv_desc;
int hvr_conv2d_nhwc(const hvr_conv_desc* d, void* stream);
/* Few-row convolutions (one 600x1000 frame gives the stride-16 stages 2 394 output pixels: 76 tiles of 128 x 64 for 256 CUs,
 * each walking the whole K = 9 Cin loop alone -- the reference's steady-state loop, tools/test.py:214-250, runs the backbone
 * on ONE new frame per output frame): bytes of caller-owned scratch with which hvr_conv2d_nhwc cuts the K loop into slices
 * (grid.y), each slice writing an f32 partial tile, followed by one reduce launch that adds bias / residual, applies the
 * ReLU and rounds once to bf16.  0 = this descriptor is not split (enough tiles, short K, f32, or a dedicated kernel takes it);
 * the call then ignores ws.  With ws == NULL or ws_bytes smaller than this the conv runs unsplit (same result up to the f32
 * summation order of the K slices).  Shapes with a short K loop (K <= 2 560, at most 320 tiles of 64 x 64) do not use the
 * workspace: their K-steps are dealt to the four waves of one workgroup per tile and summed in the LDS (csrc/kpar.hip) --
 * same contract, one launch.  HVR_CONV_SPLITK=0 in the environment turns both forms off, 2 the second one. */
size_t hvr_conv2d_splitk_workspace_bytes(const hvr_conv_desc* d);
/* Which kernel hvr_conv2d_nhwc would run for this descriptor, without launching anything (pointers are only inspected
 * for alignment): 0 = MFMA tile engine (gemm.hip), 1 = row-panel kernel for the Bottleneck's channel-expanding 1x1 conv
 * + residual (expand.hip: bf16, 1x1 stride 1, Cin = 64 / 128 / 256, a residual, Cout >= 2 Cin in whole 64-channel chunks,
 * >= 128 output pixels; tile_hint 13 forces it where it applies, HVR_EXPAND=0 in the environment turns the automatic
 * choice off), 2 = persistent 3x3 kernel with LDS-resident weights for bf16 64 -> 64 channels, stride 1, pad 1, no
 * residual (conv3x3.hip: layer 1's conv2; HVR_CONV3=0 turns it off; any tile_hint keeps the tile engine),
 * 3 = big-tile kernel (bigtile.hip: 288 x 256 output tiles, one workgroup per CU; bf16, bias / ReLU epilogue, Cout a multiple
 * of 256, K >= 512 -- taken by default when its grid covers most of the chip (>= 192 tiles: res5's and the RPN's convs on a
 * 15-frame batch), and from 96 tiles on with tile_hint 16, the hint of a caller that keeps several windows in flight and wants
 * CU-time rather than latency; bit-identical to the tile engine; HVR_BIGTILE=0 turns it off);
 * tile_hint 18 (round 6): TWO-LEVEL accumulation for exact-f32 / split-half operands whose K is a multiple of 256 elements -- every 8 K-steps'
 * products sum in a block accumulator that is then added to the running total (tile engine, 128 x 128 shape), so a long-K conv's f32 rounding noise
 * stops growing with the number of MFMAs chained on one accumulator (the RPN's 3x3 conv, K = 9 216: its share of the final boxes' distance to the
 * f64 reference halves, profiles/r06_noise_two_level.txt); other formats / shapes run as with hint 0;
 * negative = the descriptor would be rejected. */
int hvr_conv2d_path(const hvr_conv_desc* d);

/* Grouped 3x3 convolution with fused bias + ReLU: conv2 of a ResNeXt Bottleneck with its frozen BatchNorm folded in
 * (mmdet/models/backbones/resnext.py:47-56; csrc/gconv3x3.hip).  A descriptor of its own: hvr_conv_desc is unchanged.
 *   x [B][H][W][C] physical NHWC; w [C][3][3][Cg] with Cg = C / groups: output channel oc belongs to group oc / Cg and reads
 *   the input channels [g Cg, (g + 1) Cg) of that group g, w[oc][ky][kx][ci] being the weight of input channel g Cg + ci;
 *   y [B][OH][OW][C] with OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1; bias f32 [C], required; no residual:
 *     y[b][oy][ox][oc] = act( bias[oc] + sum_{ky, kx, ci} x[b][oy stride + (ky - 1) dil][ox stride + (kx - 1) dil][g Cg + ci] w[oc][ky][kx][ci] )
 *   with taps outside the map contributing zero (pad == dil) and act = ReLU when relu != 0.  f32 accumulation, ONE rounding to
 *   the stored format.
 * Instances: dtype HVR_BF16 or HVR_F16 (x, w and y share it); Cg in {4, 8, 16, 32}; C a multiple of 64, at most 2048;
 * stride 1 or 2; pad == dil, 1 or 2; x, w, y and bias 16-byte aligned; fewer than 2^31 output pixels.  A shape outside this
 * set returns HVR_EINVAL, HVR_F32 / HVR_F16S operands HVR_EUNSUPPORTED (both with a message): the caller then runs
 * hvr_conv2d_nhwc on the block-diagonal dense weight [C][3][3][C], which is the same sum with exact zeros added.  Inside a
 * 16-channel tile the kernel multiplies the inputs of neighbouring groups by exact zeros (Cg < 16), so a non-finite input
 * channel reaches the other outputs of its tile, as it would on the dense route.
 * hvr_conv3x3_grouped_supported: 1 when hvr_conv3x3_grouped runs this descriptor, else 0.  A shape query: nothing is launched,
 * pointers are inspected for alignment only. */
typedef struct hvr_gconv_desc {
  const void* x; const void* w; void* y;
  const float* bias;
  int32_t B, H, W, C, groups, stride, pad, dil;
  int32_t relu, dtype;
} hvr_gconv_desc;
int hvr_conv3x3_grouped(const hvr_gconv_desc* d, void* stream);
int hvr_conv3x3_grouped_supported(const hvr_gconv_desc* d);

/* 3x3 convolution over a channel slice of a wider NHWC map, with an optional pre-add, fused bias + ReLU: one branch of a Res2Net
 * Bottle2neck with its frozen BatchNorm folded in (mmdet/models/backbones/res2net_v1b.py:75-81; csrc/res2.hip).  A descriptor of its
 * own: hvr_conv_desc is unchanged.
 *   x, add and y are pitched maps: pixel (b, iy, ix) of x starts at element ((b H + iy) W + ix) ldx, and the slice is the Wp channels
 *   from x_off on; add (optional, NULL: none) has x's spatial size, pitch lda and slice offset add_off; y has the output's spatial size
 *   OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1, pitch ldy and offset y_off.  w [Wp][3][3][Wp], bias f32 [Wp], required:
 *     y[b][oy][ox][y_off + n] = act( bias[n] + sum_{ky, kx, c} s[b][oy stride + (ky - 1) dil][ox stride + (kx - 1) dil][c] w[n][ky][kx][c] )
 *     s[..][c] = x[..][x_off + c]                                                       when add == NULL
 *     s[..][c] = round_dtype( f32(x[..][x_off + c]) + f32(add[..][add_off + c]) )       otherwise (round to nearest even)
 *   with taps outside the map contributing zero (pad == dil) and act = ReLU when relu != 0.  f32 accumulation, ONE rounding of the
 *   result to the stored format.  Channels of x, add and y outside the slices are neither read nor written.
 * Instances: dtype HVR_BF16 or HVR_F16 (x, add, w and y share it); Wp in {32, 64, 128, 224}; stride 1 or 2; pad == dil, 1 or 2;
 * pitches and offsets multiples of 32 elements with offset + Wp <= pitch; x, add, y, w and bias 16-byte aligned; fewer than 2^31
 * output pixels; no element of y's slice may be an element of x's or add's slice (slices of ONE map at the same pitch that do not
 * share a channel are fine; any other overlap of the address ranges is refused).  A shape outside this set returns HVR_EINVAL,
 * HVR_F32 / HVR_F16S operands HVR_EUNSUPPORTED (both with a message): the caller then composes the same sum from
 * hvr_conv2d_nhwc on a contiguous copy of the slice.
 * hvr_res2_conv3x3_supported: 1 when hvr_res2_conv3x3 runs this descriptor, else 0.  A shape query: nothing is launched, pointers
 * are inspected for alignment and overlap only. */
typedef struct hvr_res2_conv_desc {
  const void* x; const void* add; void* y; const void* w;
  const float* bias;
  int64_t ldx, lda, ldy, x_off, add_off, y_off;
  int32_t B, H, W, Wp, stride, pad, dil;
  int32_t relu, dtype;
} hvr_res2_conv_desc;
int hvr_res2_conv3x3(const hvr_res2_conv_desc* d, void* stream);
int hvr_res2_conv3x3_supported(const hvr_res2_conv_desc* d);

/* Average pool over a channel slice of a pitched NHWC map (addressing as above: x / ldx / x_off -> y / ldy / y_off, C channels):
 * k x k windows, k in {1, 2, 3}, stride 1 or 2, pad <= k / 2, torch.nn.AvgPool2d's output size (ceil_mode: ceil instead of floor, and
 * the last window must start inside the map or its left padding) and divisor (count_include_pad: the window clipped to the padded
 * map, else the number of elements inside the map).  The sum runs in f32 in raster tap order, is multiplied by the f32 reciprocal
 * of the divisor and rounded once; a 1 x 1 window copies the slice bit for bit.  dtype HVR_F32, HVR_BF16 or HVR_F16 (HVR_F16S:
 * HVR_EUNSUPPORTED; pool the f32 form); C, pitches and offsets multiples of 4 with offset + C <= pitch; x and y 16-byte aligned
 * and not overlapping.  Serves a Bottle2neck's 'stage' pool (k 3, pad 1, include pad), the shortcut pool of make_res2_layer
 * (k = stride, ceil, exclude pad) and the carried slice of a 'normal' block (k 1). */
typedef struct hvr_pool_desc {
  const void* x; void* y;
  int64_t ldx, ldy, x_off, y_off;
  int32_t B, H, W, C, k, stride, pad, ceil_mode, count_include_pad, dtype;
} hvr_pool_desc;
int hvr_avgpool_nhwc(const hvr_pool_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Global context block (GCNet), forward only.  Replaces mmdet/ops/context_block.py:64-104 and the residual add + ReLU behind it
 * in a Bottleneck (resnet.py:249-264).  u [B][P][C] is a physical NHWC map (P = H * W pixels per frame) in `dtype` = HVR_F32 /
 * HVR_BF16 / HVR_F16 (HVR_F16S: HVR_EUNSUPPORTED; run the f32 form); C a multiple of 64 up to 2048, any P >= 1, any B >= 1
 * (hvr_gcb_supported answers 1 / 0 for C and dtype; anything else is refused, there is no other path).  The rule, per frame n:
 *   pool       l[p]   = sum_c u[p][c] * wm[c]                   (wm NULL, the 'avg' pooling: l = 0)
 *              a[p]   = exp(l[p] - max_q l[q]) / sum_q exp(l[q] - max_q l[q])
 *              ctx[c] = sum_p a[p] * u[p][c]
 *              (conv_mask's bias shifts every logit of a frame alike and cancels: it is not an argument)
 *   transform  h = W1 ctx + b1                                  W1 [R][C], R = int(C * ratio) >= 1
 *              g = relu((h - mean(h)) / sqrt(var(h) + 1e-5) * gamma + beta)      var = the BIASED variance over the R values
 *              o = W2 g + b2                                    passed TRANSPOSED: w2t [R][C]
 *              m[n][c] = 1 / (1 + exp(-o_mul[c]))               t[n][c] = o_add[c]
 *   apply      y = act(u * m[n][c] + t[n][c] (+ resid))         the product first, then t, then resid; act = ReLU when relu != 0
 * u is read in its stored format; everything from the logits to m and t is f32 (f32 weights, f32 accumulation); the apply is f32
 * and rounds ONCE into `dtype`.  The pool is an online softmax: the pixels of a frame are cut into S = hvr_gcb_splits(B, P, C)
 * runs (a function of the shape only), every run keeps a running maximum, sum and acc[C] that is rescaled when the maximum grows,
 * and writes ONE f32 partial (max, sum, 0, 0, acc[C]) to ws [B][S][C + 4]; the transform takes the maximum over the runs, rescales
 * and divides.  No float atomics: two runs of a call give the same bits.  An absent fusion branch is a NULL hvr_gcb_mlp pointer (and a
 * NULL m or t in the apply: m = 1, t = 0); at least one must be given.  y may be u or resid itself (same address), no other
 * overlap.  ws: hvr_gcb_workspace_bytes(B, P, C) bytes, 16-byte aligned, written by hvr_gcb_pool and read by hvr_gcb_transform on
 * the same stream.  No host synchronisation, no allocation.
 * ---------------------------------------------------------------------------------- */
typedef struct hvr_gcb_mlp {
  const float* w1; const float* b1; const float* gamma; const float* beta; const float* w2t; const float* b2;
} hvr_gcb_mlp;
int hvr_gcb_supported(int C, int dtype);
int hvr_gcb_splits(int B, int P, int C);
size_t hvr_gcb_workspace_bytes(int B, int P, int C);
int hvr_gcb_pool(const void* u, const float* wm, void* ws, size_t ws_bytes, int B, int P, int C, int dtype, void* stream);
int hvr_gcb_transform(const void* ws, size_t ws_bytes, int B, int P, int C, int R, const hvr_gcb_mlp* mul, const hvr_gcb_mlp* add, float* m,
                      float* t, void* stream);
int hvr_gcb_apply(const void* u, const float* m, const float* t, const void* resid, void* y, int B, int P, int C, int relu, int dtype,
                  void* stream);

/* ------------------------------------------------------------------------------------
 * Group normalisation (torch.nn.GroupNorm), forward only.  Replaces the norm layers that build_norm_layer makes for
 * norm_cfg = dict(type='GN', num_groups=G) (mmdet/models/utils/norm.py) behind every conv of a Bottleneck, and the residual add + ReLU
 * that close the block (resnet.py:249-264).  A GroupNorm has no running statistics: it does not fold into the conv, every map is reduced
 * per frame and group and then rescaled.  u [B][P][C] is a physical NHWC map (P = H * W pixels per frame) in `dtype` = HVR_F32 /
 * HVR_BF16 / HVR_F16 (HVR_F16S: HVR_EUNSUPPORTED; run the f32 form); G groups of Cg = C / G consecutive channels; gamma[C], beta[C] f32;
 * eps > 0.  The instance set (hvr_gn_supported answers 1 / 0 for C, G and dtype; anything else is refused before any launch, there is
 * no other path): C a multiple of 64 from 64 to 2048, G divides C, Cg in {2, 4, 8, 16, 32, 64}; any P >= 1 with P * Cg <= 2^24 (the
 * counts are exact f32 integers), any B from 1 to 65535.  The rule, per frame n and group g, over the N = P * Cg values of channels
 * [g * Cg, (g + 1) * Cg), all in f32:
 *   mean = sum u / N            var = sum (u - mean)^2 / N   (the BIASED variance)            rstd = 1 / sqrt(var + eps)
 *   a[n][c] = rstd[n][g(c)] * gamma[c]
 *   y = act((u - mean[n][g(c)]) * a[n][c] + beta[c] (+ r))       the product first, then beta, then r; act = ReLU when relu != 0
 * and each element is rounded ONCE into `dtype`.  The apply is the centred form: u * m + t with t = beta - mean * m would lose
 * |mean| * rstd * 2^-24 where a group's spread is small against its mean.  r is nothing (resid NULL), the map resid (same format and
 * shape as u), or -- ws_r, gamma_r, beta_r given -- resid normalised in the same pass, r = (resid - mean_r) * a_r + beta_r with its
 * own G-group statistics: the projection shortcut (conv, GroupNorm) of a block, whose normalised map is never written.
 * hvr_gn_stats: ONE pass.  A frame's pixels are cut into S = hvr_gn_splits(B, P, C) runs (a function of the shape only) and every run
 *  writes one f32 partial (count, mean - K, M2, K) per group to ws [B][S][G][4]: M2 = sum (u - mean)^2 over the run's values of the
 * group, K the group's PIVOT, u[n][0][g * Cg] (its first channel at the frame's first pixel).  Every value enters as u - K, an exact
 * subtraction where the group's spread is small against its mean, so no partial mean carries the mean's magnitude, and the apply
 * forms u - mean as (u - K) - (mean - K).  Partials are centred at EVERY level -- a 16-byte piece (its values of one group: the mean, then the squared distances to it), the
 * lane (a piece per pixel it visits), the wave (xor shuffles, the lower lane first), the workgroup (LDS, wave order), the runs (run
 * order, in the apply) -- and merge by Chan's formula
 *   d = mean_b - mean_a        mean = mean_a + d * n_b / n        M2 = M2_a + M2_b + d^2 * n_a * n_b / n        n = n_a + n_b
 * never through a sum of squares.  The merge order is fixed by the shape; no float atomics: two runs of a call give the same bits.
 * hvr_gn_apply: every workgroup merges the S partials of its frame (and those of ws_r) into mean and rstd, then streams 16 bytes per
 * lane.  A lane reads its pieces of u and resid before it writes the same pieces of y: y may be u or resid itself (same address), no
 * other overlap.  There is no third launch.  ws: hvr_gn_workspace_bytes(B, P, C, G) bytes, 16-byte aligned, written by hvr_gn_stats
 * and read by hvr_gn_apply on the same stream.  No host synchronisation, no allocation.
 * ---------------------------------------------------------------------------------- */
int hvr_gn_supported(int C, int G, int dtype);
int hvr_gn_splits(int B, int P, int C);
size_t hvr_gn_workspace_bytes(int B, int P, int C, int G);
int hvr_gn_stats(const void* u, void* ws, size_t ws_bytes, int B, int P, int C, int G, int dtype, void* stream);
int hvr_gn_apply(const void* u, const void* ws, const float* gamma, const float* beta, float eps, const void* resid, const void* ws_r,
                 const float* gamma_r, const float* beta_r, void* y, int B, int P, int C, int G, int relu, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Generalized (empirical) attention core, forward only.  Replaces the energy, softmax and weighted sum of
 * mmdet/models/plugins/generalized_attention.py:240-368 (spatial_range = -1, q_stride = 1); the projections in front and the closing
 * conv behind it are hvr_conv2d_nhwc calls.  q [B][H*W][heads*d], k and v [B][Hk*Wk][heads*d] are physical NHWC maps in `dtype` =
 * HVR_BF16 / HVR_F16, head m in channels [m*d, (m+1)*d); d in {16, 32, 64}, heads >= 1, Hk + Wk <= 512 (hvr_gen_attn_supported
 * answers 1 / 0; anything else is refused, the caller's other route is torch).  The rule, per frame n, head m, query pixel
 * p = (y, x) and key j = (yk, xk) = (j / Wk, j % Wk):
 *   E[p][j] = [qk] q[p] . k[j]  +  [appr_bias] appr_bias_m . k[j]
 *             + [px] q[p] . px[m][x][xk]  +  [gx] gx[m][x][xk]  +  [py] q[p] . py[m][y][yk]  +  [gy] gy[m][y][yk]
 *   A[p][.] = softmax_j E[p][.]          o[p] = sum_j A[p][j] v[j]                          (no 1 / sqrt(d) scale)
 * px [heads][W][Wk][d] and py [heads][H][Hk][d] are in `dtype`; appr_bias [heads*d], gx [heads][W][Wk] and gy [heads][H][Hk] are f32
 * (gx = geom_bias . Px and so on: the caller folds what does not depend on the frame).  A NULL pointer drops its term; q is given
 * exactly when qk or px / py are, k exactly when qk or appr_bias is.  q, k, v, px, py are read as stored; every product is accumulated
 * in f32 (the q . k and A v sums on the MFMA, the others as FMAs), the energies, the running maximum and the exp are f32.  The
 * probabilities exp(E - max) are rounded ONCE into `dtype` as the MFMA operand, and the normaliser sums those ROUNDED values in f32,
 * so a v that is constant over the keys comes back as itself; o = acc / sum is rounded ONCE into `dtype`.  The keys are taken
 * hvr_gen_attn_key_block() at a time with an online softmax (running maximum, running sum, accumulator rescaled by
 * exp(max_old - max_new)); a workgroup owns hvr_gen_attn_query_tile() consecutive pixels, which may span image rows.  E and A never
 * exist in memory.  No float atomics, a fixed order of operations: two runs of a call give the same bits.  No workspace, no host
 * synchronisation, no allocation.
 * ---------------------------------------------------------------------------------- */
typedef struct hvr_gen_attn_desc {
  const void* q; const void* k; const void* v; const float* appr_bias;
  const void* px; const void* py; const float* gx; const float* gy;
  void* o;
  int32_t B, heads, d, H, W, Hk, Wk, qk, dtype;
} hvr_gen_attn_desc;
int hvr_gen_attn_supported(int d, int heads, int Hk, int Wk, int dtype);
int hvr_gen_attn_query_tile(void);
int hvr_gen_attn_key_block(void);
int hvr_gen_attn_fwd(const hvr_gen_attn_desc* d, void* stream);

/* First conv of Res2Net's deep stem (res2net_v1b.py:174-177: Conv 3 -> 32, 3x3, stride 2, pad 1 + frozen BN + ReLU) read from the
 * f32 NCHW image img [B][3][H][W]: w f32 [32][3][3][3] as [n][ky][kx][c] and bias f32 [32] with the BN folded in; y [B][OH][OW][ldy]
 * NHWC in `dtype` (HVR_F32, HVR_BF16 or HVR_F16), OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1.  f32 FMAs, one rounding.  ldy >= 32,
 * a multiple of 4: channels 32 .. ldy - 1 of every pixel are written as exact zeros (the K padding of the conv that follows). */
int hvr_stem3x3s2_first(const float* img, const float* w, const float* bias, void* y, int B, int H, int W, int ldy, int dtype, void* stream);

/* Closing 1x1 conv of a Bottleneck whose identity path is a projection -- the first block of every stage
 * (mmdet/models/backbones/resnet.py:248-264 with `downsample`, built at resnet.py:283-296):
 *     y = relu( h W3^T + x_s Wd^T + bias )
 * in ONE pass: the downsample conv (1x1, stride s) becomes a second K segment of the expand product, so its [B][OH][OW][Cout]
 * output is neither written nor re-read as a residual.  h [B][OH][OW][C1] = conv2's output, x [B][H2][W2][C2] = the block
 * input, x_s its pixels (oy * s, ox * s); w [Cout][C1 + C2] = [W3 | Wd] rows with both BatchNorm scales folded in;
 * bias [Cout] = shift3 + shiftd (f32).  bf16; C1 + C2 in {128, 384} (stages 1 and 2 of the R-101: 64 + 64, 128 + 256) on the
 * row-panel kernel, any other C1, C2 in whole 64-channel K-steps (stage 3: 256 + 512 at stride 2, res5: 512 + 1024) on the tile engine,
 * Cout a multiple of 128.  hvr_bottleneck_tail_supported: 1 when this descriptor runs, 0 otherwise (the caller then issues the
 * two convs separately through hvr_conv2d_nhwc). */
typedef struct hvr_tail_desc {
  const void* h; const void* x; const void* w; void* y;
  int32_t B, OH, OW, C1, H2, W2, C2, stride2, Cout;
  const float* bias;
  int32_t relu, dtype;
} hvr_tail_desc;
int hvr_bottleneck_tail(const hvr_tail_desc* d, void* stream);
int hvr_bottleneck_tail_supported(const hvr_tail_desc* d);

/* The same closing 1x1 AND the next block's opening (reducing) 1x1 + bn1 + ReLU (resnet.py:224-232 of block i + 1) in one
 * pass over the pixels: the workgroup that produced all Cout channels of a pixel multiplies them by wn while they are still
 * in registers, so the next block's conv1 never re-reads y.
 *   y  = relu(h W3^T [+ x_s Wd^T] + bias [+ resid])          written as before (the next block's residual / shortcut input)
 *   hn = relu(y wn^T + bias_n)                                [B][OH][OW][Cn]
 * tail.C2 == 0 (tail.x ignored): an identity block, resid [B][OH][OW][Cout] is its input map; tail.C2 > 0: resid must be
 * NULL.  wn [Cn][Cout] bf16, bias_n f32 [Cn].  (Cout, Cn) in {(256, 64), (512, 128)}: stages 1 and 2 of the R-101;
 * hn is computed from the bf16-rounded y, exactly as a separate conv would read it. */
typedef struct hvr_tail_next_desc {
  hvr_tail_desc tail;
  const void* resid;
  const void* wn; const float* bias_n; void* hn;
  int32_t Cn;
  float alpha, beta;   /* HVR_F16S only (identity form, tail.C2 == 0, (Cout, Cn) = (256, 64)): the factors of hvr_gemm_desc on BOTH
                          products -- y = relu(alpha h W3^T + beta bias + resid), hn = relu(alpha y wn^T + beta bias_n); 0 = 1 */
} hvr_tail_next_desc;
int hvr_bottleneck_tail_next(const hvr_tail_next_desc* d, void* stream);
int hvr_bottleneck_tail_next_supported(const hvr_tail_next_desc* d);

/* The identity form of hvr_bottleneck_tail_next for a block whose output map only a stride-s consumer reads besides the next block's
 * conv1 -- the block BEFORE the last of a stage that ends compact (hvr_bottleneck_close_sampled): the last block's residual is read
 * at pixels (s oy, s ox) only, so three quarters of y are stores nobody loads.  Same products, same order:
 *   y  = relu(h W3^T + bias + resid)      computed at every pixel, WRITTEN only at pixels (s oy, s ox), as a compact map
 *                                         y [B][(OH-1)/s+1][(OW-1)/s+1][Cout]  (s = live_stride >= 1)
 *   hn = relu(y wn^T + bias_n)            [B][OH][OW][Cn], full resolution, from the rounded y in registers as before
 * tail.C2 == 0 (tail.x ignored), tail.relu == 1, resid [B][OH][OW][Cout] = the block input.  The bits of y's pixels and of all of hn
 * equal what hvr_bottleneck_tail_next writes for the same operands.  The last block then closes on (compact h, y) with
 * hvr_bottleneck_close_sampled at rstride 1 or hvr_conv2d_nhwc: a dense residual instead of a stride-s gather.
 * Dead pixels are computed (the next conv needs them) and not stored.  The kernel's vmcnt waits count the stores in flight, so its
 * instruction stream stays uniform: every wave issues every store instruction, and the lanes of dead pixels are masked out of it in EXEC
 * (a vector-memory instruction is issued and counted whatever EXEC holds).  Nothing is written outside y and hn.
 * (Cout, Cn, C1) = (256, 64, 64) / (512, 128, 128) in HVR_BF16 / HVR_F16, (256, 64, 64) in HVR_F16S (alpha / beta as in
 * hvr_tail_next_desc); B OH OW >= 128.  hvr_bottleneck_tail_next_live_supported: 1 when this descriptor runs, 0 otherwise (projection
 * blocks, exact f32, layer 3's 1024 / 256: the caller then uses hvr_bottleneck_tail_next and a full-resolution y). */
typedef struct hvr_tail_next_live_desc {
  hvr_tail_next_desc next;   /* next.tail.y: the COMPACT map */
  int32_t live_stride;
} hvr_tail_next_live_desc;
int hvr_bottleneck_tail_next_live(const hvr_tail_next_live_desc* d, void* stream);
int hvr_bottleneck_tail_next_live_supported(const hvr_tail_next_live_desc* d);

/* Closing 1x1 conv + residual + ReLU of an identity Bottleneck, computed only on the pixels a stride-s consumer reads (the last
 * block of a stage whose successor is a caffe-style stage: its first block's conv1 and downsample are both 1x1 with stride 2,
 * resnet.py:127-132,283-296, and read this block's output at pixels (s oy, s ox) only):
 *     y[b][oy][ox][:] = relu( h[b][oy][ox][:] W3^T + bias + resid[b][oy s][ox s][:] )
 * h [B][OH][OW][C1] and y [B][OH][OW][Cout] are COMPACT maps (h = the block's 3x3 conv run at stride s); resid [B][RH][RW][Cout]
 * is the block's full-resolution input, of which every s-th pixel of every s-th row is read and nothing else;
 * w [Cout][C1] with the BatchNorm scale folded in, bias f32 [Cout].  (OH - 1) s < RH and (OW - 1) s < RW.
 * Row-panel kernels only (csrc/expand.hip, csrc/expand_split.hip): HVR_BF16 / HVR_F16 / HVR_F16S, C1 = 64 or 128 (bf16 / half: also
 * 256, 512), Cout >= 2 C1 in an even number of 64-channel chunks, at least 128 output pixels.  Every output element is the sum
 * the row-panel kernel forms for the same pixel of the full-resolution product, in the same order (a panel kernel's K order does
 * not depend on M): where hvr_conv2d_nhwc takes that kernel for the full map (hvr_conv2d_path 1: C1 = 64 / 128, the closing
 * convs of layers 1 and 2) the result is bit-identical to computing the whole map and sampling it.  alpha / beta: HVR_F16S only,
 * as in hvr_gemm_desc (0 = 1).
 * hvr_bottleneck_close_sampled_supported: 1 when this descriptor runs, 0 otherwise (exact f32, fewer than 128 output pixels, other
 * channel counts: the caller then computes the block at full resolution through hvr_conv2d_nhwc). */
typedef struct hvr_close_sampled_desc {
  const void* h; const void* w; const void* resid; void* y;
  int32_t B, OH, OW, C1, Cout, RH, RW, rstride;
  const float* bias;
  int32_t relu, dtype;
  float alpha, beta;
} hvr_close_sampled_desc;
int hvr_bottleneck_close_sampled(const hvr_close_sampled_desc* d, void* stream);
int hvr_bottleneck_close_sampled_supported(const hvr_close_sampled_desc* d);

/* 7x7/2 stem: gathers img (NCHW f32, the reference's input layout, resnet.py:522-524) into
 * patch rows [B*OH*OW][KP] with k = (ky*7+kx)*3 + c and zeros for k >= 147 (KP = 192). */
int hvr_im2col_stem(const float* img, void* cols, int B, int H, int W, int KP, int dtype, void* stream);
/* Fused bf16 stem: conv1 7x7/2 (BN folded) + ReLU + MaxPool2d(3,2,1) (resnet.py:456-466,522-526) in one kernel.
 * img NCHW f32 [B][3][H][W]; wpk bf16 [64][7][32] with wpk[n][ky][kx*4+c] = w[n][c][ky][kx] (zeros for c = 3 or
 * kx = 7); bias f32 [64]; out bf16 NHWC [B][PH][PW][64], PH = ((H-1)/2+1 - 1)/2 + 1. */
int hvr_stem_fused(const float* img, const void* wpk, const float* bias, void* out, int B, int H, int W, void* stream);
/* the same in the other half formats: dtype HVR_BF16 / HVR_F16 (wpk and out in that format) or HVR_F16S -- split half: wpk is
 * [2][64][7][32] half of the weights x 2^6 (the kernel takes the factor back): plane 0 = half(64 w), plane 1 = half(64 w - plane 0); out [B][PH][PW][64] in the split-half layout */
int hvr_stem_fused_dtype(const float* img, const void* wpk, const float* bias, void* out, int B, int H, int W, int dtype, void* stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC (resnet.py:466,526) */
int hvr_maxpool3x3s2_nhwc(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Relation core:  O = softmax(scale * Q K^T, over keys) V      (single head, D up to any
 * multiple of the K-step).  Replaces torch.bmm / scalar mul / nn.Softmax / torch.mm in
 * selsa_bbox_head.py:166-182 and hrnmp_bbox_head.py:293-342 without materialising the
 * f32 Mq x Mk logits.  Q [Mq][ldq], K [Mk][ldk], V [Mk][ldv], O [Mq][ldo], all `dtype`.
 * ---------------------------------------------------------------------------------- */
size_t hvr_relation_workspace_bytes(int Mq, int Mk, int D, int dtype);
int hvr_relation_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                     void* O, int64_t ldo, int Mq, int Mk, int D, float scale, int dtype, int staging,
                     void* ws, size_t ws_bytes, void* stream);

/* The same for `groups` INDEPENDENT problems of one shape in one call -- the clips (windows) a caller has in flight, each with its
 * own Q / K / V / O: group g's operands start gs* ELEMENTS behind group 0's (a batched head keeps the groups' rows back to back in
 * one matrix: gs = rows x ld).  The reference runs one clip at a time (tools/test.py:214-250 -> hnmb_rcnn.py:195-222), so a stage of
 * W clips is W calls of the lines above; here the 352 x 256 score tiles of all groups are one list walked by persistent workgroups
 * (csrc/relation_bt.hip: HVR_BF16, HVR_F16, HVR_F16S) and, for those formats and >= 3 window-sized groups, the apply pass is one
 * launch of 288 x 256 tiles over the whole key axis (csrc/relation_apply_bt.hip).  Per group the result is hvr_relation_fwd's up to
 * the association of the f32 sums -- split half: and up to the half rounding of block-weighted probabilities below 2^-26 of a row's
 * largest -- (exact != 0: bit for bit: the scores launch stays grouped, the apply pass runs per group); shapes the grouped kernels
 * do not take run as `groups` hvr_relation_fwd calls.  Workspace: hvr_relation_grouped_workspace_bytes. */
size_t hvr_relation_grouped_workspace_bytes(int groups, int Mq, int Mk, int D, int dtype);
int hvr_relation_fwd_grouped(const void* Q, int64_t ldq, int64_t gsq, const void* K, int64_t ldk, int64_t gsk,
                             const void* V, int64_t ldv, int64_t gsv, void* O, int64_t ldo, int64_t gso, int groups,
                             int Mq, int Mk, int D, float scale, int dtype, int staging, int exact, void* ws, size_t ws_bytes, void* stream);

/* Backward of the relation core (training path; the reference gets it from autograd through
 * torch.bmm / nn.Softmax / torch.mm, selsa_bbox_head.py:166-182).  Two pieces that are not plain GEMMs:
 *   hvr_relation_probs : P = softmax(scale * Q K^T) as a [Mq][ldp] matrix in `dtype` (ldp = keys padded to 128, padding
 *                        columns zero), the f32 logits never materialised;
 *   hvr_relation_dscore: dS = scale * P * (dP - rowsum(dO * O))  (softmax backward, logit scale folded in).
 * hvr_relation_probs takes at most 16 384 keys (128 blocks of 128: its normalising sweep keeps one factor per block in a fixed
 * table); a larger Mk is HVR_EUNSUPPORTED, before anything is launched.  The same limit holds for hvr_relation_fwd /
 * hvr_relation_fwd_grouped on HVR_F16S operands whenever they normalise P in a sweep of their own (Mq >= 1024, or
 * HVR_SPLIT_NORMALIZE=1); the other relation paths fold the block factors into the apply pass and have no such limit.
 * With them  dV = P^T dO,  dP = dO V^T,  dQ = dS K,  dK = dS^T Q  are hvr_gemm / hvr_transpose_pad calls
 * (hvrnet_amd/ops.py: RelationFunction). */
size_t hvr_relation_probs_workspace_bytes(int Mq, int Mk);
int hvr_relation_probs(const void* Q, int64_t ldq, const void* K, int64_t ldk, void* P, int64_t ldp, int Mq, int Mk, int D,
                       float scale, int dtype, int staging, void* ws, size_t ws_bytes, void* stream);
int hvr_relation_dscore(const void* P, const void* dP, const void* dO, int64_t ldgo, const void* O, int64_t ldo, void* dS,
                        int Mq, int64_t ldp, int D, float scale, int dtype, void* stream);

/* Head training helpers.  The reference gets all of these from autograd:
 *   hvr_relu_bwd : dZ = dY where Y > 0 (ReLU fused into a GEMM epilogue; Y is that epilogue's output);
 *   hvr_colsum   : db[n] = sum_m dY[m][n]  (bias gradient, f32);
 *   hvr_det_loss : BBoxHead.loss for class-agnostic boxes (mmdet/models/bbox_heads/bbox_head.py:100-130 with
 *                  losses/cross_entropy_loss.py:9-20, losses/smooth_l1_loss.py:9-18, losses/accuracy.py:4-21):
 *                  out3 = (loss_cls, loss_bbox, acc) and dlogits = d(w_cls*loss_cls + w_bbox*loss_bbox)/d logits for a
 *                  logit matrix [R][ldl] holding ncls class logits at cls_off and 4 box deltas at reg_off.
 *                  PRECONDITION (also hvr_det_loss_sampled and hvr_ce_rows): every labels[r] lies in [0, ncls).  The labels are
 *                  device memory and are not range-checked (the reference's F.cross_entropy raises); a label outside the
 *                  range reads logits[r][cls_off + label], whatever lies there. */
int hvr_relu_bwd(const void* dY, const void* Y, void* dZ, int64_t n, int dtype, void* stream);
size_t hvr_colsum_workspace_bytes(int M, int N);
int hvr_colsum(const void* dY, float* db, int M, int N, int64_t ld, int dtype, void* ws, size_t ws_bytes, void* stream);
int hvr_det_loss(const float* logits, int ldl, int cls_off, int reg_off, int ncls, const int64_t* labels, const float* label_weights,
                 const float* bbox_targets, const float* bbox_weights, int R, float beta, float w_cls, float w_bbox, float* out3,
                 float* dlogits, void* stream);

/* Conv backward helpers (training path; the reference differentiates nn.Conv2d + frozen BatchNorm through autograd,
 * mmdet/models/backbones/resnet.py:220-266).  Input and weight gradients are tile-engine products:
 *   dX   = hvr_conv2d_nhwc(dZ, weights rotated 180 degrees with the channel axes swapped)      (stride-1 KxK convs)
 *   dW^T = hvr_gemm(dZ^T, cols^T)   with cols = hvr_im2col_nhwc(X): [B*OH*OW][KH*KW*Cin], stride 1, zero padding
 * hvr_scale_rows multiplies row r of a [R][C] matrix by scale[r]: the frozen BatchNorm scale folded into the weights on
 * the way in and into their gradient on the way out. */
int hvr_im2col_nhwc(const void* x, void* cols, int B, int H, int W, int Cin, int KH, int KW, int pad, int dil, int dtype, void* stream);
/* The K-contiguous operands of the weight-gradient product in one pass each (bf16 / half; round 5): colsT [KH*KW*Cin][ldt] = the
 * TRANSPOSED patch matrix (row tap*Cin + c holds that input channel of every output pixel, columns B*OH*OW .. ldt-1 zero), and
 * dZ = dY where Y > 0 together with dZt [C][ldt] = dZ^T -- instead of hvr_im2col_nhwc / hvr_relu_bwd each followed by
 * hvr_transpose_pad. */
int hvr_im2col_t(const void* x, void* colsT, int64_t ldt, int B, int H, int W, int Cin, int KH, int KW, int pad, int dil, int dtype, void* stream);
int hvr_relu_bwd_t(const void* dY, const void* Y, void* dZ, void* dZt, int64_t ldt, int R, int C, int dtype, void* stream);
int hvr_scale_rows(const void* w, const float* scale, void* out, int R, int64_t C, int dtype, void* stream);
/* The two layout + scale passes of a trainable conv in one kernel each: the f32 master weight [Cout][Cin][KH][KW] times the
 * frozen BatchNorm scale, permuted to the conv kernel's [Cout][KH][KW][Cin] and rounded to the compute dtype; and the way back
 * for the f32 weight gradient (accumulate != 0: added to `out`, i.e. written straight into the parameter's gradient buffer). */
int hvr_pack_conv_weight(const float* w, const float* scale, void* out, int Cout, int Cin, int KH, int KW, int out_dtype, void* stream);
int hvr_unpack_conv_wgrad(const float* dw, const float* scale, float* out, int Cout, int Cin, int KH, int KW, int accumulate, void* stream);
/* The weight side of a whole training iteration in two launches (round 5): `items_dev` is a table IN DEVICE MEMORY, one entry per trainable
 * conv / linear layer (pointers are stable: the parameters live in one flat buffer, dist_train.FlatParams).  hvr_pack_conv_weights_multi is
 * hvr_pack_conv_weight for every entry (first = index of the entry's first element in the concatenated work list, ascending; total = their
 * sum); hvr_transpose_multi writes dst[c][r] = src[r][c] for every entry as 64 x 64 tiles of 16-bit words (C % 8 == 0, ldd and dcols % 8 == 0,
 * columns R .. dcols - 1 of dst zero; first_tile ascending, tiles = their sum): the transposed (1x1 / linear) and the rotated (KxK, one entry per
 * filter tap) operands of the input-gradient products, from the packed weights. */
typedef struct { const float* w; const float* scale; void* out; int64_t first; int32_t Cout, Cin, KK, pad_; } hvr_pack_item;
typedef struct { const void* src; void* dst; int64_t lds, ldd; int32_t R, C, first_tile, tiles_c, dcols, pad_; } hvr_transpose_item;   /* dcols: columns of dst written per row, a multiple of 8 (R .. dcols - 1: zeros; written 8 at a time) */
int hvr_pack_conv_weights_multi(const hvr_pack_item* items_dev, int n, int64_t total, int out_dtype, void* stream);
/* hvr_unpack_conv_wgrad for a table of layers in one launch (the outputs of hvr_gemm_splitk_batched): entry i's f32 product dw [Cout][KK][Cin]
 * times scale -> the parameter-layout gradient out [Cout][Cin][KK], added to it when accumulate != 0; first / total as above. */
typedef struct { float* out; const float* scale; const float* dw; int64_t first; int32_t Cout, Cin, KK, pad_; } hvr_unpack_item;
int hvr_unpack_conv_wgrads_multi(const hvr_unpack_item* items_dev, int n, int64_t total, int accumulate, void* stream);
int hvr_transpose_multi(const hvr_transpose_item* items_dev, int n, int tiles, void* stream);

/* Optimizer step on a flat f32 buffer (the training configs: SGD lr 5e-4, momentum 0.9, weight decay 1e-4, gradient
 * clipping max_norm 35, configs/faster_rcnn_r101_selsa_c5.py:215-222; torch.optim.SGD semantics, dampening 0).  The two
 * scalings the reference applies to the summed gradient first are folded in: grad_scale = 1 / world_size
 * (mmdet/core/utils/dist_utils.py:24-25) and the clip_grad_norm_ coefficient min(1, max_norm / (norm + 1e-6)), norm taken
 * over the scaled gradient, on the device (max_norm <= 0: no clipping).  first_step: the momentum buffer is initialised
 * with the first update, as torch does. */
size_t hvr_sgd_workspace_bytes(void);
int hvr_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                 float grad_scale, float max_norm, float* ws, size_t ws_bytes, int first_step, void* stream);

/* ------------------------------------------------------------------------------------
 * RoIAlign (legacy "+1" convention).  Replaces roi_align_cuda.forward / .backward:
 *   mmdet/ops/roi_align/src/roi_align_cuda.cpp:27-80, roi_align_kernel.cu:63-141,187-282.
 * rois [K][5] f32 = (batch_idx, x1, y1, x2, y2).  layout NCHW: feat [B][C][H][W] ->
 * out [K][C][PH][PW]; layout NHWC: feat [B][H][W][C] -> out [K][PH][PW][C].
 * Backward is f32 only (as the reference) and ACCUMULATES into grad_feat (caller zeroes).
 * ---------------------------------------------------------------------------------- */
int hvr_roi_align_fwd(const void* feat, const float* rois, void* out, int B, int C, int H, int W, int K,
                      int PH, int PW, float spatial_scale, int sample_num, int dtype, int layout, void* stream);
int hvr_roi_align_bwd(const float* grad_out, const float* rois, float* grad_feat, int B, int C, int H, int W,
                      int K, int PH, int PW, float spatial_scale, int sample_num, int layout, void* stream);

/* ------------------------------------------------------------------------------------
 * Deformable im2col: the sampler of a deformable convolution (DCN v1) / modulated deformable convolution (v2), forward only.
 * Replaces mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu:63-114 (bilinear rule), :190-242 (deformable_im2col_gpu_kernel)
 * and :570-640 (modulated_deformable_im2col_gpu_kernel).
 *   x   [B][H][W][Cin]      physical NHWC, operand format `dtype` (split half: the container, activations as stored)
 *   om  [B][OH][OW][ldo]    f32, the raw output of the offset conv, pixel-major, ldo >= (modulated ? 3 : 2) * dg * KH * KW:
 *                           group g, tap k = kh * KW + kw: off_h = om[g*2*KH*KW + 2k], off_w = om[g*2*KH*KW + 2k + 1],
 *                           mask logit (modulated) = om[2*dg*KH*KW + g*KH*KW + k]; the mask is its sigmoid
 *   col [B*OH*OW][KH*KW*Cin] `dtype`, K order [kh][kw][cin] -- the order of packed conv weights [Cout][KH][KW][Cin], so the
 *                           deformable conv is hvr_gemm(col, w) with the usual epilogue.  The caller allocates it.
 * OH = (H + 2 pad - dil (KH-1) - 1) / stride + 1, OW alike.  Channel c belongs to group c / (Cin / dg).
 * Sample position h = float(oy*stride - pad + kh*dil) + off_h (one f32 add), w alike; the sample is 0 unless h > -1, w > -1,
 * h < H, w < W; else bilinear over floor and floor + 1, a corner outside the map contributing 0 (no edge clamp, unlike
 * RoIAlign); times the mask when modulated.  Interpolated in f32, rounded once to `dtype`.
 * Cin % K-step == 0 (32: f32 / split half, 64: bf16 / half) and (Cin / dg) % 8 == 0, x / col 16-byte (split half: 128-byte)
 * aligned, else HVR_EINVAL; hvr_deform_im2col_supported answers 1 / 0 for those shape rules.  No host synchronisation.
 * ---------------------------------------------------------------------------------- */
int hvr_deform_im2col_supported(int Cin, int deformable_groups, int dtype);
int hvr_deform_im2col(const void* x, const float* om, void* col, int B, int H, int W, int Cin, int KH, int KW, int stride, int pad,
                      int dil, int deformable_groups, int modulated, int64_t ldo, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Deformable (position-sensitive) RoI pooling, forward only: the pooling of DCN v1 (DeformRoIPoolingPack) / v2
 * (ModulatedDeformRoIPoolingPack).  Replaces mmdet/ops/dcn/src/deform_pool_cuda_kernel.cu:30-50 (bilinear rule), :52-140
 * (DeformablePSROIPoolForwardKernel) and the product with the mask of mmdet/ops/dcn/deform_pool.py:249-252.
 *   feat       [B][H][W][C]          physical NHWC, `dtype` = HVR_F32 / HVR_BF16 / HVR_F16 (no split-half instance)
 *   rois       [K][5]                f32 (b, x1, y1, x2, y2); b is clamped into [0, B)
 *   trans      f32 or NULL (no_trans): row n holds [ncls][2][ps][ps] (x offsets, then y offsets, per class) at row stride ldt
 *   mask_logit f32 or NULL: row n holds [P][P] at row stride ldm; the mask is its sigmoid
 *   out        [K][P][P][Cout]       `dtype`, allocated by the caller
 * P = PH = PW = out_size (square), spp = sample_per_part, gs = group_size, ps = part_size, s = spatial_scale, Cout = out_channels,
 * ncls = num_classes (1 when trans is NULL).  C == Cout * gs^2 and Cout % ncls == 0.
 * Every step is f32 and every operation is rounded on its own (no fused multiply-add).  For output (n, ct, ph, pw):
 *   rnd(v)   = round half AWAY from zero (C roundf)
 *   start_w  = rnd(x1) * s - 0.5
 *   end_w    = (rnd(x2) + 1) * s - 0.5                       h alike
 *   roi_w    = max(end_w - start_w, f32(0.1))
 *   bin_w    = roi_w / P
 *   sub_w    = bin_w / spp
 *   part_w   = floor(float(pw) / P * ps)                     part_h alike
 *   cls      = ct / (Cout / ncls)
 *   tx       = trans[n][cls][0][part_h][part_w] * trans_std
 *   ty       = trans[n][cls][1][part_h][part_w] * trans_std  (both 0 when trans is NULL)
 *   wstart   = float(pw) * bin_w + start_w
 *   wstart   = wstart + tx * roi_w                           hstart alike with ty * roi_h
 *   gw       = clamp(floor(float(pw) * gs / P), 0, gs - 1)   gh alike
 *   c        = (ct * gs + gh) * gs + gw
 *   for ih in 0..spp-1, iw in 0..spp-1 (ih outer, iw inner):
 *       w = wstart + float(iw) * sub_w
 *       h = hstart + float(ih) * sub_h
 *       skip the sample if w < -0.5 or w > W - 0.5 or h < -0.5 or h > H - 0.5
 *       w = clamp(w, 0, W - 1)
 *       h = clamp(h, 0, H - 1)
 *       xl = floor(w), xh = ceil(w), yl = floor(h), yh = ceil(h)
 *       dx = w - xl, dy = h - yl
 *       sum += (1-dx)(1-dy) v[yl][xl] + (1-dx) dy v[yh][xl] + dx (1-dy) v[yl][xh] + dx dy v[yh][xh]      (v = feat[b][.][.][c])
 *       count += 1
 *   out = 0 if count == 0 else sum / count
 *   out = out * 1 / (1 + expf(-mask_logit[n][ph][pw]))       when mask_logit is given (precise expf, rounded add and divide)
 * then ONE rounding to `dtype`.  Unlike RoIAlign: the corners are rounded, the -0.5 shift, the minimum size is 0.1, the outside
 * test is at +-0.5 with an edge clamp, ceil (not floor + 1), the divisor counts the samples inside (an empty bin gives 0), the
 * offset is indexed by PART and the mask by BIN.
 * Errors: HVR_EINVAL for a non-square out_size, C != Cout * gs^2, Cout % ncls != 0, trans_std outside [0, 1], ldt < ncls*2*ps*ps,
 * ldm < P*P, a split-half dtype, null or misaligned pointers.  No host synchronisation, no allocation.
 * ---------------------------------------------------------------------------------- */
int hvr_deform_roi_pool_fwd(const void* feat, const float* rois, const float* trans, const float* mask_logit, void* out, int B, int H, int W,
                            int C, int K, int PH, int PW, int out_channels, int group_size, int part_size, int num_classes,
                            int sample_per_part, float spatial_scale, float trans_std, int64_t ldt, int64_t ldm, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * RoI max pooling with its argmax backward (RoIPool).  Replaces mmdet/ops/roi_pool/src/roi_pool_kernel.cu:16-74 (forward) and
 * :112-135 (backward).
 *   feat     [B][H][W][C]        physical NHWC, `dtype` = HVR_F32 / HVR_BF16 / HVR_F16 (split half: HVR_EUNSUPPORTED, pool in f32)
 *   rois     [K][5]              f32 (b, x1, y1, x2, y2), as RoIAlign
 *   out      [K][PH][PW][C]      `dtype`, allocated by the caller
 *   argmax   [K][PH][PW][C]      int32 or NULL (the inference form: no index is kept or written)
 * Every geometry step is one f32 operation, rounded on its own (no fused multiply-add), s = spatial_scale:
 *   rx1 = x1 * s                 ry1 = y1 * s
 *   rx2 = (x2 + 1) * s           ry2 = (y2 + 1) * s
 *   rw  = rx2 - rx1              rh  = ry2 - ry1
 *   bw  = rw / PW                bh  = rh / PH
 *   bin (ph, pw):  xs = floor(float(pw) * bw + rx1)    xe = ceil(float(pw + 1) * bw + rx1)
 *                  ys = floor(float(ph) * bh + ry1)    ye = ceil(float(ph + 1) * bh + ry1)
 *   each clamped to [0, W] resp. [0, H] as a float, then converted to int
 *   out    = max of feat[b][h][w][c] over ys <= h < ye, xs <= w < xe
 *   argmax = h * W + w of the FIRST pixel in row-major order (h outer, w inner) that attains it
 * This is roi_pool_kernel.cu:30-56 with scalar_t = float.  What differs from the reference:
 *   geometry dtype  f32 for every feature dtype (the reference computes it in half for half maps);
 *   clamp           on the float, before the conversion to int: any finite coordinate is safe;
 *   selection       stated as "first pixel that attains the maximum" (values compared after an exact widening to f32, the
 *                   stored result is the input element).  The reference starts at `first - 1` under a strict `>` and selects the
 *                   same pixel wherever x - 1 < x; the rule here needs no subtraction and so holds for large bf16 values too.
 *                   Inputs are finite; NaN is unspecified;
 *   empty bin       xe <= xs or ye <= ys: value 0 and argmax -1 for every channel;
 *   malformed RoI   rw <= 0 or rh <= 0: all bins value 0 and argmax -1 (the reference leaves argmax 0 there and its backward adds
 *                   the gradient to pixel 0);
 *   batch index     b outside [0, B) (compared as a float, else truncated): the RoI is treated as malformed and no memory is
 *                   read for it (the reference reads out of bounds);
 *   backward        grad_feat[b][argmax][c] += grad_out[k][ph][pw][c] for every output element with argmax >= 0; nothing happens
 *                   for -1 (the reference writes one element before the plane there).
 * Contraction changes bins: at s = 1/16, PW = 7, W = 11 the last bin of x1 = -39, x2 = 31 is [1, 2) as stated and [1, 3) with a
 * fused multiply-add; x1 = -39, x2 = 95: [4, 6) against [4, 7); x1 = -37, x2 = 15: [0, 1) against [0, 2).
 * Forward: C % 8 == 0 (2-byte dtypes) / C % 4 == 0 (f32), else HVR_EUNSUPPORTED; feat, out, argmax 16-byte aligned.  K == 0 returns
 * without a launch.  Backward: f32 only, ACCUMULATES into grad_feat [B][H][W][C] with f32 atomics (the caller zeroes it); of rois
 * only the batch index is read.  Non-positive PH, PW, H, W, C or negative K, B: HVR_EINVAL.  No host synchronisation, no allocation.
 * ---------------------------------------------------------------------------------- */
int hvr_roi_pool_fwd(const void* feat, const float* rois, void* out, int32_t* argmax /* may be NULL */, int B, int H, int W, int C, int K,
                     int PH, int PW, float spatial_scale, int dtype, void* stream);
int hvr_roi_pool_bwd(const float* grad_out, const float* rois, const int32_t* argmax, float* grad_feat, int B, int H, int W, int C, int K,
                     int PH, int PW, void* stream);

/* ------------------------------------------------------------------------------------
 * FPN top-down merge, one launch, out of place.  Replaces the L - 1 steps
 *   laterals[i - 1] += F.interpolate(laterals[i], scale_factor=2, mode='nearest')
 * of mmdet/models/necks/fpn.py:117-120 (an upsample launch and an add launch each).
 *   lat[l]   [B][H[l]][W[l]][C]   physical NHWC, `dtype` = HVR_F32 / HVR_BF16 / HVR_F16, l = 0 (finest) .. L - 1 (coarsest)
 *   out[l]   [B][H[l]][W[l]][C]   `dtype`, for l < L - 1; out[L - 1] is never read: the top level's merged map is its lateral
 * lat, out, H, W are host arrays of L entries.  H[l] == 2 * H[l + 1] and W[l] == 2 * W[l + 1] exactly (what scale_factor=2 produces;
 * the reference raises on anything else).  The rule, in f32:
 *   m[L - 1]            = lat[L - 1]
 *   m[j][b][h][w][c]    = lat[j][b][h][w][c] + m[j + 1][b][h >> 1][w >> 1][c]
 *   out[l][b][h][w][c]  = lat[l][b][h][w][c] + m[l + 1][b][h >> 1][w >> 1][c]        rounded to `dtype` ONCE
 * i.e. the sum is associated from the coarsest level inwards, the reference's order, and no level reads another level's rounded
 * output (the composite rounds a 16-bit level once per add, up to three times at L = 4; in f32 both give the same bits).
 * 16 bytes of channels per lane, no atomics, no workspace, no host synchronisation; workgroups need no order.
 * Instances (hvr_fpn_merge_supported answers 1 / 0): 1 <= L <= HVR_FPN_MAX_LEVELS; C a multiple of 8 (2-byte dtypes) / of 4 (f32), at most
 * 65536; not split half (merge the f32 laterals).  Outside the set: HVR_EUNSUPPORTED.  A size mismatch, a non-positive size, a null
 * or not 16-byte aligned map, or an out[l] whose bytes overlap any lat[j] or another out[j]: HVR_EINVAL.  Every refusal comes before
 * any launch and nothing is written.  L == 1 or B == 0 succeeds without a launch.
 * ---------------------------------------------------------------------------------- */
#define HVR_FPN_MAX_LEVELS 4
int hvr_fpn_merge_supported(int L, int C, int dtype);
int hvr_fpn_merge(const void* const* lat, void* const* out, int L, int B, const int32_t* H, const int32_t* W, int C, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * RoIAlign over up to four NHWC maps of one batch in ONE launch: each RoI is pooled on the map its size selects.  Replaces the loop
 * of mmdet/models/roi_extractors/single_level.py:89-107 (map_roi_levels :55-73, one `inds.any()` host read per level, gather, pool,
 * scatter into a zeroed output).  No host read, no workspace, no zero-fill pass; a level without RoIs costs nothing.
 * Level of RoI k, from rois[k] = (b, x1, y1, x2, y2), in f32, every operation rounded on its own (no fused multiply-add; the
 * division and the square root correctly rounded):
 *   w = (x2 - x1) + 1
 *   h = (y2 - y1) + 1
 *   s = sqrt(w * h)
 *   v = s / finest_scale + 1e-6f
 *   level = [v >= 2] + [v >= 4] + ... + [v >= 2^(L-1)]
 * This is floor(log2(v)) clamped to [0, L - 1] without a transcendental.  It differs from torch's own evaluation only where torch's
 * log2f rounds a value just below a power of two up to it: on a CPU with finest_scale = 56 that happened in 1 of 2 000 000 random
 * float boxes, in 0 of 2 000 000 integer-sized boxes and in none of the boundary boxes (squares of side 56 * 2^k, 112 x 111,
 * 111 x 113, 224 x 224, 223 x 225).  A NaN v (exactly one side negative) fails every comparison: level 0.  (The reference's
 * .long() of NaN is platform-defined: no level on the CPU, level 0 on CUDA.)
 * Pooling: out[k] is what hvr_roi_align_fwd writes for pool_rois[k] (layout NHWC) on map `level` with that level's H, W and
 * spatial_scale -- the same device code, bit for bit, the sample_num == 2 form of the 2-byte dtypes included.  pool_rois == rois
 * unless the boxes are rescaled for pooling (roi_scale_factor); the batch index of pool_rois[k] selects the frame and must lie in
 * [0, B), as for hvr_roi_align_fwd.
 * Instances (hvr_roi_align_levels_supported answers 1 / 0): 1 <= L <= HVR_FPN_MAX_LEVELS, dtype HVR_F32 / HVR_BF16 / HVR_F16 (split half:
 * HVR_EUNSUPPORTED, pool in f32), C a multiple of 4 up to 1024 -- the set of the single-map call.  Maps and out 16-byte aligned
 * (2-byte dtypes: 8-byte; the 16-byte form is taken when all are 16-byte aligned), rois / pool_rois / levels 4-byte.  Bad shapes,
 * null or misaligned pointers, finest_scale <= 0: HVR_EINVAL, before any launch.  K == 0 succeeds without a launch.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const void* feat[HVR_FPN_MAX_LEVELS];      /* [B][H[l]][W[l]][C], entries l >= L ignored */
  int32_t H[HVR_FPN_MAX_LEVELS], W[HVR_FPN_MAX_LEVELS];
  float spatial_scale[HVR_FPN_MAX_LEVELS];   /* 1 / stride of the level */
  int32_t L, B, C, K, PH, PW, sample_num, dtype;
  float finest_scale;                        /* 56 in the reference's configs */
  const float* rois;                         /* [K][5] decide the level */
  const float* pool_rois;                    /* [K][5] are pooled (== rois without a roi_scale_factor) */
  void* out;                                 /* [K][PH][PW][C] */
  int32_t* levels;                           /* [K] or NULL: the level of every RoI */
} hvr_roi_levels_desc;
int hvr_roi_align_levels_supported(int L, int C, int dtype);
int hvr_roi_align_levels_fwd(const hvr_roi_levels_desc* d, void* stream);

/* ------------------------------------------------------------------------------------
 * Greedy NMS.  Replaces nms_cpu.nms / nms_cuda.nms (mmdet/ops/nms/src/nms_cpu.cpp:5-71,
 * nms_kernel.cu:24-136) with no host round trip.  dets [n][5] f32 (x1,y1,x2,y2,score);
 * ge_semantics != 0 suppresses at IoU >= thr (the CPU reference), 0 at IoU > thr (the CUDA
 * reference).  keep [n] int64 receives the surviving indices in ascending input order,
 * *n_keep their count (both device memory).  n <= 8192.
 * ---------------------------------------------------------------------------------- */
size_t hvr_nms_workspace_bytes(int n);
int hvr_nms(const float* dets, int n, float thr, int ge_semantics, int64_t* keep, int32_t* n_keep,
            void* ws, size_t ws_bytes, void* stream);
/* The same, stopping after the first max_keep survivors in score order: `nms(proposals, thr)[:nms_post]` of
 * mmdet/models/anchor_heads/rpn_head.py:95-97 without pricing the IoUs of boxes behind the cut.  keep: ascending input
 * order of those survivors.  One workgroup that evaluates only the rows of surviving boxes (max_keep x n IoUs, not n^2/2);
 * max_keep <= 1024, larger caps take the mask + sweep path of hvr_nms and stop the sweep at the cap. */
int hvr_nms_first(const float* dets, int n, float thr, int ge_semantics, int max_keep, int64_t* keep, int32_t* n_keep,
                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * RPN proposal generation for T frames in one call.  Replaces RPNHead.get_bboxes_single
 * (mmdet/models/anchor_heads/rpn_head.py:55-104) + AnchorGenerator.grid_anchors
 * (mmdet/core/anchor/anchor_generator.py:66-83) + delta2bbox (core/bbox/transforms.py:78-110):
 * sigmoid, top nms_pre, decode + clip, NMS(thr, >=), first nms_post, top max_num by score.
 *   cls [T][H][W][A] f32 logits, reg [T][H][W][A*4] f32 (NHWC conv outputs),
 *   base_anchors host [A][4] f32, means/stds host [4] f32.
 *   proposals [T][max_num][5] f32, counts [T] int32 (rows beyond counts[t] are untouched).
 * T >= 1, A >= 1, nms_post > 0 and max_num > 0 (else HVR_EINVAL, nothing launched); nms_pre <= 0 means no top-k.
 * ---------------------------------------------------------------------------------- */
typedef struct hvr_rpn_desc {
  const float* cls; const float* reg;
  int32_t T, H, W, A, anchor_stride;
  const float* base_anchors; const float* means; const float* stds;  /* host */
  float img_h, img_w, wh_ratio_clip;
  int32_t nms_pre, nms_post, max_num;
  float nms_thr;
  float* proposals; int32_t* counts;
  int32_t cls_pitch, reg_pitch;  /* channels per pixel of the cls / reg maps (0 = A / 4A); lets both be
                                    channel slices of one fused [T][H][W][5A(+pad)] conv output */
} hvr_rpn_desc;
size_t hvr_rpn_workspace_bytes(int T, int H, int W, int A, int nms_pre);
int hvr_rpn_proposals(const hvr_rpn_desc* d, void* ws, size_t ws_bytes, void* stream);
/* Calls with T <= frames take the chip-wide kernels (histogram / counting-sort selection, banded suppression mask + one-wave
 * sweep: many workgroups per frame) instead of one workgroup per frame; the proposals are the same bit for bit.  Default 4
 * (HVR_RPN_WIDE=<frames> in the environment overrides it; 0 = never).  frames < 0 only queries.  Returns the previous value.
 * PROCESS-WIDE (an atomic): every thread and device of the process sees the new value from its next call on. */
int hvr_rpn_wide_frames(int frames);

/* ------------------------------------------------------------------------------------
 * Guided Anchoring RPN (GA-RPN), inference only, one level.  Replaces the inference path of GuidedAnchorHead / GARPNHead
 * (mmdet/models/anchor_heads/guided_anchor_head.py:197-208, :271-362; ga_rpn_head.py:60-127) and MaskedConv2dFunction.forward
 * (mmdet/ops/masked_conv/masked_conv.py:15-53).  Every step is f32 and every operation of the mask, offset and box rules is
 * rounded on its own (no fused multiply-add); expf is the precise one, add and divide are correctly rounded.
 *
 * hvr_ga_mask_offsets: the location mask and the offset conv (feature_adaption.conv_offset) in one launch.
 *   loc    [T][H][W] f32 logits, one per pixel, at pixel pitch loc_pitch (>= 1) -- a channel slice of a wider conv output is fine
 *   keep   [T][H][W] uint8:  s = 1 / (1 + expf(-loc));  keep = (s >= loc_filter_thr) ? 1 : 0        (guided_anchor_head.py:203, :343-345)
 *   shape  [T][H][W][2] f32 at pixel pitch shape_pitch (>= 2)
 *   w_off  [nch][2] f32, the 1x1 offset conv's weight (no bias), nch = deformable_groups * 2 * KH * KW
 *   om     [T][H][W][ldo] f32, ldo >= nch:  om[c] = w_off[c][0] * shape[0] + w_off[c][1] * shape[1]   (two products, one add)
 *          -- the layout hvr_deform_im2col reads; columns nch .. ldo are not written
 * keep == NULL computes only the offsets, om == NULL only the mask (both NULL: HVR_EINVAL).  The masked conv and the proposal
 * entry below both READ this one keep map, so they cannot disagree about a pixel.
 *
 * hvr_masked_conv_fwd: conv evaluated at the kept pixels only.
 *   x    [B][H][W][Cin]       physical NHWC, HVR_BF16 / HVR_F16 / HVR_F32 (HVR_F16S: HVR_EUNSUPPORTED; run the f32 form)
 *   w    [Cout][KH][KW][Cin]  the packed conv layout, same dtype;  bias [Cout] f32 or NULL
 *   keep [B][H][W] uint8      one mask PER FRAME (the reference asserts batch 1 and takes frame 0's mask: this is the per-frame
 *                             generalisation, equal to the reference at B = 1)
 *   out  [B][H][W][ldo] f32, ldo >= Cout; columns Cout .. ldo are not written
 *   keep != 0:  out[co] = bias[co] + sum over (kh, kw, ci) of x[b][y - pad + kh][x - pad + kw][ci] * w[co][kh][kw][ci]
 *               (taps outside the map contribute nothing), accumulated in f32 in a fixed order, rounded once
 *   keep == 0:  out[co] = 0 exactly, for all Cout channels (NOT the bias: new_zeros + scatter, masked_conv.py:37-52); the rows
 *               of x under an unkept pixel are not read
 * Stride 1, KH == KW odd, pad == (KH - 1) / 2 (else HVR_EINVAL); Cin a multiple of 8 (f32: 4), x and w 16-byte aligned.
 * Cout <= hvr_masked_conv_max_cout() (8): a skinny product with one wave per pixel; above it HVR_EUNSUPPORTED (run the dense
 * conv and zero the unkept pixels).  No atomics: the same bits on every call.
 *
 * hvr_ga_rpn_proposals: guided anchors + proposal read-out for T frames.  Per frame, with n = H * W pixels in row-major order:
 *   1. candidates = the pixels with keep == 1, in row-major order
 *   2. square  = base_square + (x * stride, y * stride, x * stride, y * stride); base_square is the grid anchor of
 *                AnchorGenerator(base_size, [octave_base_scale], [1.0]) (host [4] f32)
 *      anchor  = delta2bbox(square, (0, 0, shape[0], shape[1]), anchoring_means, anchoring_stds, wh_ratio_clip = 1e-6), no
 *                max_shape -- the means are added to dx and dy too
 *   3. score   = 1 / (1 + expf(-cls))
 *   4. nms_pre > 0 and more than nms_pre candidates: the top nms_pre by score (equal scores: lower pixel index first)
 *   5. box     = delta2bbox(anchor, reg, target_means, target_stds, wh_ratio_clip) clipped to [0, img_w - 1] x [0, img_h - 1]
 *   6. NMS at nms_thr with the IoU >= thr rule of hvr_rpn_proposals; of the survivors the first nms_post IN THE ORDER OF THE
 *      CANDIDATE LIST -- score order when step 4 took a top-k, row-major pixel order when it did not (the reference's CPU NMS returns
 *      the survivors by ascending input index; hvr_rpn_proposals reads it the same way) -- then the top max_num of those by score
 *   delta2bbox(a, d, m, s, clip): d = d * s + m; dw, dh clamped to +-|log(clip)|; px = (a.x1 + a.x2) * 0.5, pw = a.x2 - a.x1 + 1;
 *      gw = pw * expf(dw); gx = px + pw * dx; x1 = gx - gw * 0.5 + 0.5; x2 = gx + gw * 0.5 - 0.5; y alike
 *   cls [T][H][W] (pitch cls_pitch), reg [T][H][W][4] (reg_pitch), shape [T][H][W][2] (shape_pitch): f32, may be channel slices
 *   of fused conv outputs (pitch 0 = dense: 1 / 4 / 2); keep [T][H][W] uint8 from hvr_ga_mask_offsets.
 *   proposals [T][max_num][5] f32 in score order, counts [T] int32 (rows beyond counts[t] are untouched).
 * A frame with no kept pixel gives counts[t] = 0 (the reference `continue`s past the level and then fails in torch.cat).
 * One form: one workgroup per frame selects, the mask + sweep NMS kernels of hvr_nms suppress (no survivor cap: step 6).  H * W <= 8192 (the C4 map of a
 * 1000 x 600 frame, 38 x 63, has 2 394), nms_post <= 4096, else HVR_EUNSUPPORTED; T >= 1, nms_post > 0, max_num > 0, a finite
 * wh_ratio_clip > 0, else HVR_EINVAL.  Nothing synchronises with the host, nothing allocates: the whole head can be captured in a graph.
 * ---------------------------------------------------------------------------------- */
int hvr_ga_mask_offsets(const float* loc, int64_t loc_pitch, float loc_filter_thr, uint8_t* keep, const float* shape, int64_t shape_pitch,
                        const float* w_off, float* om, int64_t ldo, int nch, int64_t pixels, void* stream);
int hvr_masked_conv_max_cout(void);
int hvr_masked_conv_fwd(const void* x, const void* w, const float* bias, const uint8_t* keep, float* out, int B, int H, int W, int Cin,
                        int Cout, int KH, int KW, int pad, int64_t ldo, int dtype, void* stream);
typedef struct hvr_ga_rpn_desc {
  const float* cls; const float* reg; const float* shape; const uint8_t* keep;
  int32_t T, H, W, anchor_stride;
  int32_t cls_pitch, reg_pitch, shape_pitch;   /* floats per pixel of each map (0 = 1 / 4 / 2) */
  const float* base_square;                    /* host [4] */
  const float* anchoring_means; const float* anchoring_stds; const float* target_means; const float* target_stds;  /* host [4] */
  float img_h, img_w, wh_ratio_clip;           /* wh_ratio_clip of step 5 (16 / 1000); step 2 always uses 1e-6 */
  int32_t nms_pre, nms_post, max_num;
  float nms_thr;
  float* proposals; int32_t* counts;
} hvr_ga_rpn_desc;
size_t hvr_ga_rpn_workspace_bytes(int T, int H, int W, int nms_pre);
int hvr_ga_rpn_proposals(const hvr_ga_rpn_desc* d, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * RCNN detection read-out for one key frame.  Replaces BBoxHead.get_det_bboxes
 * (mmdet/models/bbox_heads/bbox_head.py:132-169; hrnmp_bbox_head.py:1009-1052 per branch):
 *   hvr_det_decode:     softmax over classes + delta2bbox + clip (+ / scale_factor)
 *   hvr_multiclass_nms: mmdet/core/post_processing/bbox_nms.py:6-66 (class-agnostic boxes)
 * logits [R][ldl] f32 with class logits at cls_off.. and 4 deltas at reg_off..;
 * rois [R][5]; scores [R][ncls]; boxes [R][4]; dets [max_num][5]; labels [max_num] int64
 * (0-based foreground class); *n_out device int32; rows [*n_out, max_num) of dets / labels come back zeroed (R > 0:
 * the caller's buffers need no initialisation).
 * hvr_multiclass_nms: max_num > 0 (else HVR_EINVAL); R <= 512, 1 .. 128 foreground classes (ncls - 1) and
 * (ncls - 1) * R <= 16384 -- the merge keeps the whole candidate list, next_pow2((ncls - 1) * R) entries of 8 bytes, in LDS;
 * 30 classes x 512 rows fit, 128 x 512 do not -- (else HVR_EUNSUPPORTED); nothing is launched and nothing written on an error.
 * hvr_multiclass_nms_workspace_bytes returns 0 for a shape outside that envelope.  R == 0 writes only the count (zero).
 * scale_factor <= 0 means rescale=False.  img_w <= 0 means no clipping.
 * ---------------------------------------------------------------------------------- */
int hvr_det_decode(const float* logits, int ldl, int cls_off, int reg_off, int ncls, const float* rois, int R,
                   const float* means, const float* stds, float wh_ratio_clip, float img_h, float img_w,
                   float scale_factor, float* scores, float* boxes, void* stream);
size_t hvr_multiclass_nms_workspace_bytes(int R, int ncls);
int hvr_multiclass_nms(const float* boxes, const float* scores, int R, int ncls, float score_thr, float iou_thr,
                       int max_num, float* dets, int64_t* labels, int32_t* n_out, void* ws, size_t ws_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * Soft-NMS read-out (test_cfg.rcnn.nms type='soft_nms').  Replaces soft_nms (mmdet/ops/nms/nms_wrapper.py:64-102) +
 * soft_nms_cpu (mmdet/ops/nms/src/soft_nms_cpu.pyx:22-127) and multiclass_nms around it
 * (mmdet/core/post_processing/bbox_nms.py:32-61, which resolves the operator by name) with no host round trip: the reference
 * goes to numpy once per class (nms_wrapper.py:77-79).  method 1 = linear (weight 1 - IoU above iou_thr), 2 = gaussian
 * (weight exp(-IoU^2 / sigma)); entries whose rescored value falls below min_score leave the list.  The arithmetic is the
 * compiled .pyx's mix of f32 and f64 (hvrnet_amd/csrc/softnms.hip).
 *   hvr_soft_nms:            dets [n][5] f32 (x1,y1,x2,y2,score) -> out_dets [n][5] = the kept boxes with their RESCORED scores in
 *                            selection order, inds [n] int64 their input indices, *n_out the count (device int32); rows behind it
 *                            are zeroed.  n <= 512.
 *   hvr_multiclass_soft_nms: P >= 1 independent problems in one launch pair.  boxes [P][R][4], scores [P][R][ncls] (column 0 =
 *                            background).  Per foreground class the rows with score > score_thr (ascending row) go through
 *                            soft-NMS; the classes' lists (selection order, rescored scores) are concatenated in class order
 *                            and, if more than max_num remain, cut to the max_num highest rescored scores (descending; equal
 *                            scores: lower position in the concatenated list).  dets [P][max_num][5], labels [P][max_num] int64
 *                            (0-based foreground class), n_out [P] device int32; rows behind n_out[p] come back zeroed.
 *                            R <= 512, at most 128 foreground classes, max_num > 0.  R == 0 (and n == 0 above) writes only the
 *                            counts (zero): dets / labels / inds are not touched.
 * ---------------------------------------------------------------------------------- */
size_t hvr_soft_nms_workspace_bytes(int n);
int hvr_soft_nms(const float* dets, int n, float iou_thr, int method, float sigma, float min_score, float* out_dets, int64_t* inds,
                 int32_t* n_out, void* ws, size_t ws_bytes, void* stream);
size_t hvr_multiclass_soft_nms_workspace_bytes(int P, int R, int ncls);
int hvr_multiclass_soft_nms(const float* boxes, const float* scores, int P, int R, int ncls, float score_thr, float iou_thr, int method,
                            float sigma, float min_score, int max_num, float* dets, int64_t* labels, int32_t* n_out, void* ws,
                            size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Seq-NMS read-out of ONE whole video (Han et al. 2016; the reference tree has none: DESIGN.md holds the specification and
 * tests/seqnms_refs.py its host restatement).  boxes [F][R][4] (x1,y1,x2,y2, +1 pixel convention, class-agnostic), scores
 * [F][R][ncls] (column 0 = background), the F key frames in time order; padding rows carry score 0 in every column.
 * Per foreground class: candidates = rows with score > score_thr; (t,i) links to (t+1,j) iff IoU >= link_thr; repeat until no
 * candidate is alive { best[t,i] = s[t,i] + max over alive linked j of best[t+1,j] (0 if none), backward in time; root = alive
 * box with the largest best (lowest t, then lowest i); the path follows the lowest j attaining the max; every path box gets the
 * score best[root] / n (rescore 1 = avg) or the path's largest score (rescore 2 = max), is kept and retired, and so is -- but
 * dropped -- every alive box of its frame with IoU >= nms_thr to it }.  IoU = the f32 arithmetic of nms_cpu.cpp.
 * Output per frame as hvr_multiclass_nms: kept rows class-major, ascending row, with the rescored scores; cut to the max_num
 * highest (descending, list position ascending on ties) if more are kept; dets [F][max_num][5], labels [F][max_num] int64
 * (0-based), n_out [F] int32, rows behind n_out[t] zeroed.  F = 1 equals hvr_multiclass_nms(score_thr, nms_thr) row for row.
 * F >= 1, score_thr >= 0, max_num > 0 (else HVR_EINVAL); R <= 512, F <= 65535, at most 128 foreground classes and
 * (ncls - 1) * R <= 16384 -- the merge keeps a frame's whole candidate list, next_pow2((ncls - 1) * R) entries of 8 bytes, in
 * LDS; 30 classes x 512 rows fit, 128 x 512 do not -- (else HVR_EUNSUPPORTED); nothing is launched on an error.  R == 0 writes only the counts (zero).  Three launches on `stream`, no
 * host read: capturable.
 *   hvr_seq_nms_phases: UNSTABLE measurement hook, not part of the supported interface (it may change or go without an ABI
 *                       bump): the same call restricted to the kernels named in `phases` (1 link / overlap bits, 2 per-class
 *                       paths, 4 per-frame merge; 7 = hvr_seq_nms), for timing a kernel alone (tools/seqnms_bench.py).  Phases 2
 *                       and 4 read what the earlier phases of the SAME arguments left in `ws`: if anything else wrote that
 *                       workspace in between, the result is undefined (no check is possible).  Products call hvr_seq_nms.
 * ---------------------------------------------------------------------------------- */
size_t hvr_seq_nms_workspace_bytes(int F, int R, int ncls);
int hvr_seq_nms(const float* boxes, const float* scores, int F, int R, int ncls, float score_thr, float link_thr, float nms_thr,
                int rescore, int max_num, float* dets, int64_t* labels, int32_t* n_out, void* ws, size_t ws_bytes, void* stream);
int hvr_seq_nms_phases(const float* boxes, const float* scores, int F, int R, int ncls, float score_thr, float link_thr, float nms_thr,
                       int rescore, int max_num, float* dets, int64_t* labels, int32_t* n_out, void* ws, size_t ws_bytes, int phases,
                       void* stream);
/* Several problems per launch and tube outputs: the same kernels, hvr_seq_nms being their P = 1, no-tubes case.
 * A problem is one video's key frames for one read-out branch: problem p owns the frames frame_start[p] .. frame_start[p+1]-1 of
 * boxes [Ftot][R][4] / scores [Ftot][R][ncls]; frame_start is a DEVICE int32 [P+1] array the caller builds (frame_start[0] = 0,
 * frame_start[P] = Ftot, every problem at least one frame; the kernels clamp what they read from it to 0 .. Ftot).  Nothing crosses
 * a problem boundary: dets / labels / n_out ([Ftot]...) are, problem by problem, bit-identical to P calls of hvr_seq_nms on the slices.
 * Tube outputs (all four pointers NULL = none; any other mix: HVR_EINVAL): every selected path is a tube (singletons count), ids are
 * problem-local, 0-based, class-major and within a class in selection order.  tube_ids [Ftot][max_num] int32: the tube of each
 * output row, -1 behind n_out[t].  The table is concatenated problem-major, then in id order: tubes [max_tubes][4] int32 =
 * (problem, 0-based label, start frame relative to the problem, length -- the boxes selected on the path, also those the per-frame
 * max_num cut removed from their frame's list), tube_scores [max_tubes] f32 the rescored value of every member, tube_start [P+1]
 * int32 the prefix counts (tube_start[P] = the true total).  Only the first min(total, max_tubes) rows are written, the rows
 * behind stay untouched; tube_start and all ids stay exact.  The table is 16-byte aligned.
 * Limits as hvr_seq_nms, and P >= 1, Ftot >= P, max_tubes >= 0 with tubes (else HVR_EINVAL), Ftot <= 65535 (else HVR_EUNSUPPORTED);
 * nothing is launched on an error.  R == 0 writes only the counts (n_out, tube_start: zero).  Three launches on `stream` (four
 * with tubes), no host read: capturable. */
size_t hvr_seq_nms_batched_workspace_bytes(int P, int Ftot, int R, int ncls, int tubes);
int hvr_seq_nms_batched(const float* boxes, const float* scores, int P, const int32_t* frame_start, int Ftot, int R, int ncls, float score_thr,
                        float link_thr, float nms_thr, int rescore, int max_num, float* dets, int64_t* labels, int32_t* n_out,
                        int32_t* tube_ids, int32_t* tubes, float* tube_scores, int32_t* tube_start, int max_tubes, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- layout / dtype plumbing at the API boundary ---- */
/* any pair of the four dtypes; pairs other than f32 <-> bf16 move 8 elements per thread: n % 8 == 0 and 16-byte aligned buffers
 * (split half: n % 32 == 0 -- a contiguous tensor whose last dimension is a multiple of 32 -- and 128-byte alignment) */
int hvr_cast(const void* in, void* out, int64_t n, int from_dtype, int to_dtype, void* stream);
/* out = convert(in * scale), scale > 0 (a power of two for exact results): how the host layer moves between true values and the
 * scaled split-half tensors it keeps (activations x 2^4, weights x 2^6: hvrnet_amd/native.py) */
int hvr_cast_scaled(const void* in, void* out, int64_t n, int from_dtype, int to_dtype, float scale, void* stream);
/* to_nhwc != 0: [B][C][HW] -> [B][HW][C]; else the inverse */
int hvr_permute_nchw_nhwc(const void* in, void* out, int B, int C, int HW, int to_nhwc, int from_dtype,
                          int to_dtype, void* stream);
/* out[C][ldt] = in[R][ldx]^T, zero-filled for columns >= R */
int hvr_transpose_pad(const void* in, void* out, int R, int C, int64_t ldx, int64_t ldt, int dtype, void* stream);

/* Training targets: ground truth -> assigned, sampled boxes -> loss targets, all on the device.
 *   hvr_max_iou_assign : MaxIoUAssigner.assign (mmdet/core/bbox/assigners/max_iou_assigner.py:48-173, IoU of
 *                        mmdet/core/bbox/geometry.py:46-60) for float thresholds, gt_max_assign_all=True and no ignore
 *                        boxes: gt_inds[i] = -1 ignore / 0 background / g+1 assigned to gt g; max_overlaps[i].
 *                        `valid` (nullable, one byte per box) marks the boxes that take part: anchor_target_single's
 *                        inside_flags (mmdet/core/anchor/anchor_target.py:104-112) without compacting the anchors;
 *                        boxes outside get gt_inds -1 and max_overlaps -1.  n == 0 or k == 0 is HVR_EINVAL where the
 *                        reference raises ValueError('No gt or bboxes').
 *   hvr_sample_pos_neg : BaseSampler.sample (mmdet/core/bbox/samplers/base_sampler.py:32-78) over boxes classed by
 *                        cls[i] (> 0 positive, == 0 negative, < 0 neither).  From each class the boxes with the
 *                        smallest keys[i] win (ties: lower index); RandomSampler = uniform random keys
 *                        (random_sampler.py:37-53 shuffles on the host instead), OHEMHNLSampler.get_ohem_weights =
 *                        keys -loss (ohem_hnl_sampler.py:50-113).  inds[0..counts[0]) positives, then counts[1]
 *                        negatives, each ascending -- SamplingResult's order (sampling_result.py:9-12 after .unique()).
 *                        Keys compare numerically (-0.0 ties with +0.0, +-inf are ordinary values); NaN keys are
 *                        unspecified.  Rows of inds behind counts[0] + counts[1] are not written.  neg_pos_ub < 0: no
 *                        cap; otherwise at most int(neg_pos_ub * max(1, counts[0])) negatives, the product taken in
 *                        double on the caller's double as base_sampler.py:70 takes it (a float argument would round
 *                        0.29 x 100 up to 29 where the reference gets 28).
 *   hvr_box_targets    : regression / classification targets of the sampled boxes (transforms.py:6-31 bbox2delta).
 *                        scatter = 1: [n]-row outputs, row inds[j]  (anchor_target.py:121-155 after `unmap`);
 *                        scatter = 0: [num]-row outputs, row j      (bbox_target.py:35-62).  gt_labels null: label 1.
 *   hvr_rpn_loss       : AnchorHead.loss_single for one level, sigmoid objectness (anchor_head.py:141-160 with
 *                        losses/cross_entropy_loss.py:23-37 and losses/smooth_l1_loss.py:9-18) on the fused RPN head
 *                        output o [rows][ldo] (A logits then 4A deltas per position): out2 = (loss_rpn_cls,
 *                        loss_rpn_bbox), d_o = d(sum of both)/d o, every element written (columns 5A .. ldo: zero);
 *                        avg_factor = max(counts[0],1) + max(counts[1],1).
 *   hvr_ce_rows        : per-row softmax cross entropy (`reduction_override='none'`, selsa_rcnn.py:209-218); labels in
 *                        [0, ncls), unchecked (see hvr_det_loss).
 *   hvr_det_loss_sampled: hvr_det_loss in the OHEM form (selsa_rcnn.py:224-232): rows outside cat(pos_inds, neg_inds)
 *                        carry zero weights; smooth-L1 and the accuracy are averaged over sel_counts[0]+sel_counts[1]
 *                        (at least 1); labels in [0, ncls), unchecked (see hvr_det_loss). */
size_t hvr_max_iou_assign_workspace_bytes(int n, int k);
int hvr_max_iou_assign(const float* boxes, int ldb, int n, const float* gts, int k, const uint8_t* valid, float pos_iou_thr,
                       float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int64_t* gt_inds, float* max_overlaps, void* ws,
                       size_t ws_bytes, void* stream);
int hvr_sample_pos_neg(const int64_t* cls, const float* keys, int n, int num, int num_expected_pos, double neg_pos_ub, int64_t* inds,
                       int32_t* counts, void* stream);
int hvr_box_targets(const float* boxes, int ldb, int n, const float* gts, const int64_t* gt_labels, const int64_t* gt_inds,
                    const int64_t* inds, const int32_t* counts, int num, const float* means4, const float* stds4, float pos_weight,
                    int scatter, int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights, void* stream);
int hvr_rpn_loss(const float* o, int ldo, int A, int rows, const int64_t* labels, const float* label_weights, const float* bbox_targets,
                 const float* bbox_weights, const int32_t* counts, float beta, float* out2, float* d_o, void* stream);
int hvr_ce_rows(const float* logits, int ldl, int cls_off, int ncls, const int64_t* labels, int R, float* loss, void* stream);
/* Hard-proposal mining of the HVR head (mmdet/models/bbox_heads/hrnmp_bbox_head.py:357-414 `hardest_proposal_mining`): for
 * every query row of the scaled affinity matrix aff [Mq][ld] (f32), with row label labels[r] and key labels all_labels[k]:
 *   out4[r][0] argmax over keys with a different label  (the reference's masked_fill(-inf) + topk(1), `inds_for_pos_sm`)
 *   out4[r][1] argmin over keys with the same label     (masked_fill(+inf) + topk(1, largest=False), `inds_for_pos_nsm`)
 *   out4[r][2], out4[r][3] the two largest among keys with a different label (topk(2), `inds_for_bg`, used for label-0 rows)
 * ties to the lower index; a row without candidates gets index 0 (0, 1); a row with one candidate gets the lowest other index as
 * its second pick (0 when Mk == 1).  +-inf affinities are ordinary values.  NaN affinities are unspecified: the kernel never selects
 * one, whereas the reference's topk ranks NaN highest. */
/* STAND-IN for the triplet loss over the mined triples: the reference calls TripletNonLocalLoss(margin).compute_loss(q, k, labels,
 * [anchor_idx, pos_idx, neg_idx]) (hrnmp_bbox_head.py:555-561) from a pytorch_metric_learning fork that is NOT in the reference tree.
 * This is the library's published TripletMarginLoss with anchors from q and positives / negatives from k:
 * d(x,y) = ||x - y + 1e-6||_2, l_i = max(d(q_a,k_p) - d(q_a,k_n) + margin, 0), loss = sum l_i / max(#{l_i > 0}, 1).
 * out2 = (loss, number of active triples); dq [Mq][D] / dk [Mk][D] (f32, nullable) = d loss / d q, d k.  ws: 3 n floats. */
int hvr_triplet_margin(const void* q, int64_t ldq, const void* k, int64_t ldk, int D, int Mq, int Mk, const int64_t* anchor_idx,
                       const int64_t* pos_idx, const int64_t* neg_idx, int n, float margin, int dtype, float* ws, size_t ws_bytes,
                       float* out2, float* dq, float* dk, void* stream);
int hvr_mining_argreduce(const float* aff, int Mq, int Mk, int64_t ld, const int64_t* labels, const int64_t* all_labels, int64_t* out4,
                         void* stream);
int hvr_det_loss_sampled(const float* logits, int ldl, int cls_off, int reg_off, int ncls, const int64_t* labels,
                         const float* label_weights, const float* bbox_targets, const float* bbox_weights, int R,
                         const int32_t* sel_counts, float beta, float* out3, float* dlogits, void* stream);

/* ------------------------------------------------------------------------------------
 * Sigmoid focal loss (mmdet/ops/sigmoid_focal_loss/src/sigmoid_focal_loss_cuda.cu:24,62 SigmoidFocalLossForward / Backward,
 * mmdet/models/losses/focal_loss.py, losses/utils.py weight_reduce_loss).  THE RULE, stated once: x is a logit, p = sigmoid(x); row n
 * of N has the int64 target t[n]; column c of C is POSITIVE iff t == c + 1, NEGATIVE iff t >= 0 and t != c + 1, and contributes
 * NOTHING (loss 0, gradient 0) iff t < 0 (the reference's c1 / c2; t = 0 is background):
 *   positive:  l = -alpha     (1-p)^gamma log p         dl/dx = -alpha     (1-p)^gamma (1 - p - gamma p log p)
 *   negative:  l = -(1-alpha) p^gamma     log(1-p)      dl/dx = -(1-alpha) p^gamma     (gamma (1-p) log(1-p) - p)
 * gamma >= 0 and 0 <= alpha <= 1, anything else is HVR_EINVAL before any launch.  All math is f32 through the stable forms
 *   e = expf(-|x|), log p = min(x,0) - log1pf(e), log(1-p) = -max(x,0) - log1pf(e), p and 1-p = 1/(1+e) and e/(1+e) by the sign of x,
 *   q^gamma = expf(gamma log q) on the log already formed (so q^0 = 1 also where q underflows to 0, as powf gives),
 * with the device library's expf / log1pf, not the fast intrinsics.  The result is finite for every finite x.  DEVIATION: the
 * reference clamps log p at log FLT_MIN once p underflows (x < -87.3, where its loss stops growing at 87.3 alpha); this build
 * follows the mathematical value there (the loss goes on as -alpha x).
 * Reduction (weight_reduce_loss): a per-row weight w[n] multiplies all C columns of the row (focal_loss.py:39-41); 'none' is the
 * [N, C] matrix, 'sum' its sum, 'mean' the sum divided by N C, or by avg_factor when one is given; then times loss_weight.
 *   hvr_sigmoid_focal_loss_fwd : logits [N][ldl] (HVR_F32 / HVR_BF16 / HVR_F16; HVR_F16S is refused), row pitch ldl >= C in elements,
 *                        targets int64 [N] -> loss f32 [N][C].
 *   hvr_sigmoid_focal_loss_bwd : the same inputs and d_loss f32 [N][C] -> d_logits f32 [N][C] = dl/dx * d_loss.
 *   hvr_focal_loss     : the reduced form on f32 logits in ONE pass over them: out1[0] = (sum_n w[n] sum_c l[n][c]) * (loss_weight / avg)
 *                        and d_logits [N][ldl] = (loss_weight / avg * w[n]) * dl/dx, every element written (columns C .. ldl: zero).
 *                        w is nullable (all ones).  avg is the host float `avg` (> 0), or, when counts_dev (int32, nullable) is given,
 *                        max(counts_dev[0], 1) read on the device.  The sum is deterministic: S = hvr_focal_loss_splits workgroups of
 *                        consecutive rows (a function of the shape only, none empty), per-lane partials in row-then-column order, xor
 *                        shuffles, the four waves through LDS in wave order, ONE f32 partial per workgroup into ws
 *                        (hvr_focal_loss_workspace_bytes), the partials merged in workgroup order by one wave (lane i takes i, i + 64,
 *                        ...; xor shuffles).  No float atomics: two calls give the same bits.
 *   hvr_rpn_focal_loss : hvr_rpn_loss's contract (o [rows][ldo] = A objectness logits then 4A deltas, out2 = (loss_rpn_cls,
 *                        loss_rpn_bbox), d_o fully written, columns 5A .. ldo zero) for a sampling-free head (anchor_head.py:62): the
 *                        classification term is the rule above with C = 1, target = label, row weight = label_weights, per anchor;
 *                        BOTH terms divide by max(counts[0], 1), the positive count (anchor_head.py:194-195, anchor_target.py:66);
 *                        w_cls / w_bbox are the loss_weight of either term.  The smooth-L1 element is hvr_rpn_loss's own.
 * 16 bytes per lane where pitch and addresses allow, a scalar form otherwise (any ldl works); no host synchronisation and no
 * allocation: every entry point can be captured in a graph.  N * ldl < 2^31.
 * ---------------------------------------------------------------------------------- */
int hvr_sigmoid_focal_loss_fwd(const void* logits, int ldl, const int64_t* targets, int N, int C, float gamma, float alpha, int dtype,
                               float* loss, void* stream);
int hvr_sigmoid_focal_loss_bwd(const void* logits, int ldl, const int64_t* targets, const float* d_loss, int N, int C, float gamma,
                               float alpha, int dtype, float* d_logits, void* stream);
int hvr_focal_loss_splits(int N, int C);
size_t hvr_focal_loss_workspace_bytes(int N, int C);
int hvr_focal_loss(const float* logits, int ldl, const int64_t* targets, const float* w, int N, int C, float gamma, float alpha,
                   float loss_weight, float avg, const int32_t* counts_dev, void* ws, size_t ws_bytes, float* out1, float* d_logits,
                   void* stream);
int hvr_rpn_focal_loss(const float* o, int ldo, int A, int rows, const int64_t* labels, const float* label_weights,
                       const float* bbox_targets, const float* bbox_weights, const int32_t* counts, float beta, float gamma, float alpha,
                       float w_cls, float w_bbox, float* out2, float* d_o, void* stream);

/* ------------------------------------------------------------------------------------
 * Regression and IoU losses (mmdet/models/losses/smooth_l1_loss.py, balanced_l1_loss.py, mse_loss.py, iou_loss.py, with
 * losses/utils.py weight_reduce_loss).  THE RULES, stated once; all math is f32, every product and sum rounded on its own, with the
 * device library's logf / log1pf, not the fast intrinsics.
 * Elementwise family (hvr_reg_*): pred f32 [N][ldp] (row pitch ldp >= D in elements); target, the optional weight, the loss and the
 * gradient are dense f32 [N][D].  d = pred - target, a = |d|, sign(0) = 0:
 *   HVR_REG_SMOOTH_L1 (beta):    l = a < beta ? 0.5 a a / beta : a - 0.5 beta          dl/dpred = a < beta ? d / beta : sign(d)
 *   HVR_REG_BALANCED_L1 (alpha, gamma, beta), b = e^(gamma / alpha) - 1 formed in f64 from the three floats and rounded once:
 *       a < beta:   l = alpha / b (b a + 1) log(b a / beta + 1) - alpha a
 *                   dl/dpred = (alpha log(b a / beta + 1) + alpha (1 - beta) / (b a + beta)) sign(d)
 *       otherwise:  l = gamma a + gamma / b - alpha beta                                dl/dpred = gamma sign(d)
 *     The gradient is the derivative of l as stated, which is what the reference's autograd gives; its second term vanishes
 *     (exactly, in f32 too) at beta = 1, where the gradient is the paper's alpha log(b a + 1).
 *     log(y + 1) is log1pf(y): DEVIATION in the accurate direction (the reference forms y + 1 first and loses y's low bits).
 *   HVR_REG_MSE:                 l = d d                                                dl/dpred = 2 d
 *     DEVIATION: the reference's mse_loss wraps F.mse_loss, whose own default reduction averages BEFORE weight_reduce_loss sees the
 *     elements (mse_loss.py:7), so there only the unweighted 'mean' is the mean of d d; this build applies weight and reduction to the
 *     elements, as weighted_loss states its contract.
 *   beta, alpha, gamma are ignored by the rules that do not name them.
 * Box-pair family (hvr_box_*): pred, target dense f32 [n][4] = x1, y1, x2, y2 with the legacy "+1" widths; gradient [n][4], to pred only.
 *   HVR_BOX_IOU (eps):  I = max(min(x2) - max(x1) + 1, 0) max(min(y2) - max(y1) + 1, 0), iou = I / (A_pred + A_target - I) as
 *     bbox_overlaps(is_aligned=True) forms it; l = -log(max(iou, eps)), ONE value and ONE weight per pair (loss, weight: [n]).  The
 *     gradient is zero where iou < eps; elsewhere dl = dU / U - dI / I.  Where the two sides of a max / min tie, PRED takes the
 *     gradient.  DEVIATION: a NaN iou (both boxes of zero area) gives l = -log eps with a zero gradient, not NaN.
 *   HVR_BOX_BOUNDED_IOU (beta, eps):  per axis, with centres c = (x1 + x2) / 2, sizes s = x2 - x1 + 1 and dx = c_t - c_p:
 *       centre term  1 - max((s_t - 2|dx|) / (s_t + 2|dx| + eps), 0)      size term  1 - min(s_t / (s_p + eps), s_p / (s_t + eps))
 *     in the order (dx, dy, dw, dh) (iou_loss.py:41-58); each term c goes through c < beta ? 0.5 c c / beta : c - 0.5 beta.  The loss and
 *     the weight are [n][4], per element.  Ties: the ZERO takes the gradient of the max; the FIRST ratio (s_t / (s_p + eps)) that of the min.
 * Forms of both families:
 *   *_fwd : the 'none' loss.      *_bwd : d_pred = dl/dpred * d_loss (d_loss in the loss's shape).
 *   hvr_reg_loss / hvr_box_loss : the reduced form in ONE pass over the inputs: out1[0] = (sum w l) * (loss_weight / avg) and
 *     d_pred = (loss_weight / avg * w) dl/dpred, every element written.  w is nullable (all ones); all-zero weights give exactly 0
 *     through the sum itself (the reference's torch.any early exit would be a host read and is not reproduced).  avg is the host
 *     float `avg` (> 0), or, when counts_dev (int32, nullable) is given, max(counts_dev[0], 1) read on the device.  The sum follows the
 *     focal scheme: S = hvr_reg_loss_splits(N, D) / hvr_box_loss_splits(n) workgroups of consecutive rows (a function of the shape
 *     only, none empty), per-lane partials in row-then-column order, xor shuffles, the four waves through LDS in wave order, ONE f32
 *     partial per workgroup into ws (S floats: hvr_*_workspace_bytes), the partials merged in workgroup order by one wave.  No float
 *     atomics: two calls give the same bits.
 * 16 bytes per lane where pitch and addresses allow, a scalar form otherwise; no host synchronisation and no allocation: every entry
 * point can be captured in a graph.  N * ldp < 2^31, n < 2^29.
 * ---------------------------------------------------------------------------------- */
enum { HVR_REG_SMOOTH_L1 = 0, HVR_REG_BALANCED_L1 = 1, HVR_REG_MSE = 2 };
enum { HVR_BOX_IOU = 0, HVR_BOX_BOUNDED_IOU = 1 };
int hvr_reg_loss_fwd(int rule, const float* pred, int ldp, const float* target, int N, int D, float beta, float alpha, float gamma, float* loss,
                     void* stream);
int hvr_reg_loss_bwd(int rule, const float* pred, int ldp, const float* target, const float* d_loss, int N, int D, float beta, float alpha,
                     float gamma, float* d_pred, void* stream);
int hvr_reg_loss_splits(int N, int D);
size_t hvr_reg_loss_workspace_bytes(int N, int D);
int hvr_reg_loss(int rule, const float* pred, int ldp, const float* target, const float* w, int N, int D, float beta, float alpha, float gamma,
                 float loss_weight, float avg, const int32_t* counts_dev, void* ws, size_t ws_bytes, float* out1, float* d_pred, void* stream);
int hvr_box_loss_fwd(int rule, const float* pred, const float* target, int n, float beta, float eps, float* loss, void* stream);
int hvr_box_loss_bwd(int rule, const float* pred, const float* target, const float* d_loss, int n, float beta, float eps, float* d_pred,
                     void* stream);
int hvr_box_loss_splits(int n);
size_t hvr_box_loss_workspace_bytes(int n);
int hvr_box_loss(int rule, const float* pred, const float* target, const float* w, int n, float beta, float eps, float loss_weight, float avg,
                 const int32_t* counts_dev, void* ws, size_t ws_bytes, float* out1, float* d_pred, void* stream);

/* ------------------------------------------------------------------------------------
 * GHM losses (mmdet/models/losses/ghm_loss.py GHMC / GHMR).  THE RULES, stated once.  Inputs are dense f32 [N][C], taken as E = N C
 * elements; the weight is [N][C] (or [N], one per row, when weight_per_row: the labels form below).  An element is VALID iff its
 * weight is above 0.  Per element:
 *   GHMC: x the logit, t the target; p = sigmoid(x) in focal's stable forms (e = expf(-|x|), p = 1 / (1 + e) or e / (1 + e));
 *         g = |p - t|;   term = max(x, 0) - x t + log1pf(expf(-|x|));   slope = p - t.
 *         t is the float target [N][C], or with int64 labels [N] the rule of _expand_binary_labels: label k >= 1 marks column k - 1.
 *   GHMR: d = pred - target, r = sqrtf(d d + mu mu);   g = |d / r|;   term = r - mu;   slope = d / r.
 * `edges` f32 [bins + 1] (1 <= bins <= 64) belongs to the caller; a valid element falls into bin i iff edges[i] <= g < edges[i + 1]
 * (an element outside every bin counts towards tot and carries no loss).  One call runs three passes and reads nothing on the host:
 *   0. the counts are zeroed by a one-wave launch of their own (a kernel, not a memset node: the call is meant to be captured).
 *   1. histogram: counts[i] per workgroup in LDS with integer atomics, one integer atomic per bin and workgroup into counts (exact
 *      whatever the order).  tot = max(., 1) of: GHMC the NUMBER of valid elements (integer sum); GHMR the SUM OF ALL WEIGHTS, as the
 *      reference has it (f32, in the deterministic order of the reduced losses over S = hvr_ghm_splits(N, C) workgroups of consecutive
 *      elements).
 *   2. finalize, one wave: n = the number of non-empty bins; per non-empty bin, with momentum > 0: acc_sum[i] = momentum acc_sum[i] +
 *      (1 - momentum) counts[i] IN PLACE and beta_i = tot / acc_sum[i], otherwise beta_i = tot / counts[i]; w[i] = beta_i / n.
 *      Empty bins leave acc_sum[i] untouched and have w[i] = 0.
 *   3. loss and gradient in one pass (bin weights are constants of the gradient): out1[0] = loss_weight * (sum w[bin] term) / tot,
 *      d[e] = loss_weight * w[bin] * slope / tot, zero for invalid elements; the sum as in the reduced losses (one partial per
 *      workgroup, merged in order by a one-wave launch).
 * Workspace (hvr_ghm_workspace_bytes), in 4-byte words, left behind for the caller to read: [0, 64) counts int32; [64, 128) w f32;
 * [128] tot f32; [129] n int32; [192, 192 + S) the workgroups' partials.  No float atomics, no allocation: capturable in a graph (a
 * replay with momentum > 0 advances acc_sum once).  N C < 2^31.
 * ---------------------------------------------------------------------------------- */
int hvr_ghm_splits(int N, int C);
size_t hvr_ghm_workspace_bytes(int N, int C);
int hvr_ghmc_loss(const float* logits, const float* target, const int64_t* labels, const float* weight, int weight_per_row, int N, int C,
                  const float* edges, int bins, float momentum, float* acc_sum, float loss_weight, void* ws, size_t ws_bytes, float* out1,
                  float* d_logits, void* stream);
int hvr_ghmr_loss(const float* pred, const float* target, const float* weight, int N, int C, float mu, const float* edges, int bins,
                  float momentum, float* acc_sum, float loss_weight, void* ws, size_t ws_bytes, float* out1, float* d_pred, void* stream);

/* Frame ingest: decoded BGR uint8 frame src [src_h][src_pitch bytes] (3 bytes per pixel) -> dst f32 [3][pad_h][pad_w]:
 * bilinear resize to new_w x new_h (OpenCV's 8-bit INTER_LINEAR fixed-point arithmetic, which mmcv.imrescale calls), optional
 * BGR->RGB, (x - mean) / std, zero padding -- the reference's Resize -> Normalize -> Pad -> ImageToTensor
 * (mmdet/datasets/pipelines/transforms.py:111-124,260-269,308-313) in one kernel instead of three CPU passes per frame. */
int hvr_ingest_frame(const uint8_t* src, int src_h, int src_w, int64_t src_pitch, float* dst, int new_h, int new_w, int pad_h, int pad_w,
                     const float* mean3, const float* std3, int to_rgb, void* stream);
/* The same with RandomFlip(horizontal) in its place between Resize and Pad (transforms.py:190-196, the flip=True half of a
 * MultiScaleFlipAug test pipeline, mmdet/datasets/pipelines/test_aug.py): flip != 0 mirrors the resized new_h x new_w image, the
 * zero padding stays on the right and at the bottom.  flip == 0 is hvr_ingest_frame bit for bit. */
int hvr_ingest_frame_flip(const uint8_t* src, int src_h, int src_w, int64_t src_pitch, float* dst, int new_h, int new_w, int pad_h, int pad_w,
                          const float* mean3, const float* std3, int to_rgb, int flip, void* stream);

/* ------------------------------------------------------------------------------------
 * Test-time augmentation (multi-scale / flip): the box plumbing between the per-augmentation stages of
 * HNMBRCNN.forward_feat_aug / aug_test_bboxes (mmdet/models/detectors/hnmb_rcnn.py:104-180, 640-698) for all T frames of a
 * window, with no host read.  An augmentation a is (img_w[a], scale_factor[a], flip[a]): HOST arrays of A entries, 1 <= A <= 16.
 * Un-flip / flip: x1' = img_w - x2 - 1, x2' = img_w - x1 - 1; back = (un-flip, then a true division by scale_factor), forward =
 * (times scale_factor, then flip) -- bbox_mapping_back / bbox_mapping of mmdet/core/bbox/transforms.py:114-146.
 *   hvr_merge_aug_proposals: merge_aug_proposals (mmdet/core/post_processing/merge_augs.py:8-44) per frame, one launch for the
 *                       window: proposals [A][T][mx][5] f32 of which rows < counts[a][t] ([A][T] int32, device) are valid ->
 *                       mapped back, concatenated in augmentation order, greedy NMS at IoU >= nms_thr (nms_cpu semantics),
 *                       survivors by descending score (ties: lower concatenated index), the first max_num of them:
 *                       merged [T][max_num][5] in original-image coordinates, rows behind merged_counts[t] ([T] int32, device)
 *                       zeroed.  A * mx <= 8192, max_num <= 4096.  One workgroup per frame.
 *   hvr_map_aug_rois:   bbox_mapping + bbox2roi (transforms.py:131-136,149-168 as hnmb_rcnn.py:645-651 uses them: ONE img_w /
 *                       scale_factor / flip per augmentation, the key frame's, for all frames): merged [T][max_num][5] ->
 *                       rois [A][T * max_num][5] = (frame index, box in augmentation a's coordinates).
 *   hvr_merge_aug_dets: merge_aug_bboxes (merge_augs.py:47-70): boxes [A][R][4] (each in its augmentation's coordinates, i.e.
 *                       hvr_det_decode with scale_factor = 0) and scores [A][R][ncls] -> merged_boxes [R][4] = mean over a of the
 *                       boxes mapped back, merged_scores [R][ncls] = mean over a (sums in augmentation order, one division by A).
 *                       Feeds hvr_multiclass_nms (R <= 512 there).
 * ---------------------------------------------------------------------------------- */
size_t hvr_merge_aug_proposals_workspace_bytes(int A, int T, int mx);
int hvr_merge_aug_proposals(const float* proposals, const int32_t* counts, int A, int T, int mx, const float* img_w,
                            const float* scale_factor, const int32_t* flip, float nms_thr, int max_num, float* merged,
                            int32_t* merged_counts, void* ws, size_t ws_bytes, void* stream);
int hvr_map_aug_rois(const float* merged, int A, int T, int max_num, const float* img_w, const float* scale_factor, const int32_t* flip,
                     float* rois, void* stream);
int hvr_merge_aug_dets(const float* boxes, const float* scores, int A, int R, int ncls, const float* img_w, const float* scale_factor,
                       const int32_t* flip, float* merged_boxes, float* merged_scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HVR_HIP_H_ */
