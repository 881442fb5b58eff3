/* unidepth_hip.h -- C-ABI of the MI355X (gfx950) kernel library behind UniDepthV2.infer().
 *
 * The reference has no FFI on this path: every op below replaces a torch call made by the reference's
 * Python modules (file:line relative to the reference tree).  Conventions mirror the reference's own
 * native-op convention (unidepth/ops/extract_patches/src/extract_patches.cpp:3-6, ops/knn/src/knn.cu:130,330-341)
 * minus the torch types: raw device pointers + sizes, the caller owns every buffer (incl. workspace),
 * work is enqueued on the hipStream_t passed in (`void* stream`; NULL = default stream), no hidden
 * allocation, no host sync.  Return value: 0 = OK, negative = UD_ERR_* (the Python side raises RuntimeError).
 * All functions are stateless and re-entrant; one process per GPU.
 *
 * Activations are fp16 (MFMA operands) or fp32 (residual streams, statistics, outputs); weights are fp16,
 * [N, K] row-major with K contiguous and K padded to a multiple of 64 (zeros).
 */
#ifndef UNIDEPTH_HIP_H
#define UNIDEPTH_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UD_OK 0
#define UD_ERR_BAD_ARG (-1)
#define UD_ERR_LAUNCH (-2)
#define UD_ERR_UNSUPPORTED (-3)

/* ---- GEMM epilogues ------------------------------------------------------------------------------- */
#define UD_EPI_F16 0   /* out(fp16)[row, n] = act(acc + bias[n] + add[.., n])                                      */
#define UD_EPI_F32 1   /* out(fp32)[row, n] (+)= acc + bias[n] + add[.., n], then `act` (NONE / GELU / CLAMPEXP) on the stored value;
                        * optional fp16 copy out2 = act2(result)  */
#define UD_EPI_QKV 2   /* n <  vsplit: out(fp16) row-major;  n >= vsplit: out2(fp16) = V^T [img][head][64][kv_ld], the 4-key blocks
                        * of every aligned 16-key group stored in the order [0, 2, 1, 3] (= the k-slot order of the P V MFMA,
                        * so the attention kernel DMAs V^T tiles to LDS as they are): key t lives at column
                        * (t & ~15) | ((t & 4) << 1) | ((t & 8) >> 1) | (t & 3)                                                       */
#define UD_EPI_D2S 3   /* ConvTranspose(k=s) depth-to-space: out(fp32 NHWC) += acc + bias[o]; out2 fp16 = act2(..)   */
#define UD_EPI_HEAD 4  /* y = sum_n lrelu(acc + bias[n]) * w2[n] + b2;  out(fp32)[m] = exp(clip(y,-8,8) + post_add) */

#define UD_ACT_NONE 0
#define UD_ACT_GELU 1   /* exact erf GELU (nn.GELU default; reference metadinov2/mlp.py:35-41, layers/mlp.py:27) */
#define UD_ACT_LRELU 2  /* LeakyReLU(0.01) (reference layers/upsample.py:164) */
#define UD_ACT_CLAMPEXP 3  /* exp(clamp(x, -10, 10)) (UniDepthV1 multi-scale outputs, unidepthv1/decoder.py:322-325); UD_EPI_F32 `act` only */

#define UD_A_DENSE 0          /* A is [M, lda] row-major                                              */
#define UD_A_CONV3_ZERO 1     /* A rows are gathered 3x3 taps of an NHWC image, zero padding           */
#define UD_A_CONV3_REFLECT 2  /* same, reflect padding (reference decoder.py:199-226)                   */
#define UD_A_CONV3_REFLECT_UP 3  /* reflect-padded 3x3 taps of the bilinear align_corners=True up-sampling of A [B, Hsrc, Wsrc, Cin] to
                                  * (Himg, Wimg) (decoder.py:299-301,309-311 fused into the following conv; UD_EPI_HEAD only); img_stride and gA
                                  * describe the LOW-resolution A */

/* C[M,N] = A[M,K] * W[N,K]^T on v_mfma_f32_16x16x32_f16 tiles, fp32 accumulate.
 * Replaces: nn.Linear / F.linear everywhere on the path (metadinov2/attention.py:53,60; mlp.py:36-40;
 * layers/attention.py:117-122,139; layers/mlp.py:30-33; decoder.py:44,145), the patch-embed Conv2d
 * (metadinov2/patch_embed.py:66-88), ConvTranspose2d (decoder.py:166-173), 3x3/1x1 Conv2d
 * (layers/upsample.py:148-163,208-214; decoder.py:199-226) as implicit GEMMs. */
/* UdGemm.tile_hint.  A forced schedule that is not eligible for the descriptor falls back as noted; 4 and values above 14 are unassigned. */
#define UD_HINT_AUTO 0            /* the cost model decides (csrc/gemm.hip route()) */
#define UD_HINT_TILE128 1         /* 128-row tiles only: no large-tile, no halo-tile schedule */
#define UD_HINT_LIST256 2         /* 256 x 256 tile list */
#define UD_HINT_LIST192 3         /* 192 x 256 tile list (dense A: with the 3-deep weight ring) */
#define UD_HINT_PLAIN128 5        /* 128 x 128 tiles, plain 2-stage kernel */
#define UD_HINT_RING 6            /* 128 x 128 tiles, 4-stage pipelined ring without the K split (what auto picks when the tile count is at most
                                   * the CU count and K >= 512) */
#define UD_HINT_RING_SPLITK 7     /* 6 + the two-way K split across CUs (splitk_ws / splitk_cnt; K >= 512 instead of auto's 1024) */
#define UD_HINT_BALANCED 8        /* row-balanced schedule of the 256-column kernel (auto picks it when the tile list would leave the last round
                                   * partly empty); not eligible -> auto */
#define UD_HINT_LIST192_W2 9      /* 192 x 256 tile list with the 2-deep weight ring (dense 192-row launches otherwise fetch the weight operand two
                                   * K-tiles ahead through a 3-deep LDS ring: same bits, the weights of a layer are cold in every step) */
#define UD_HINT_LIST192_SPLITK 10 /* 192 x 256 tiles with the two-way K split of the large-tile list (splitk_ws_bytes); refused -> 128-row tiles */
#define UD_HINT_PINGPONG 11       /* 192 x 256 tiles in the ping-pong form (csrc/gemm_pp.hip; UD_EPI_F32, dense); refused -> 192 x 256 tile list */
#define UD_HINT_DUO_FIRST 12      /* 192 x 128 tiles, two workgroups per CU (csrc/gemm_pp.hip), the first-dispatched workgroup of a CU at high priority; */
#define UD_HINT_DUO_EQUAL 13      /*   the same with equal priorities; */
#define UD_HINT_DUO_SECOND 14     /*   the same with the second-dispatched one at high priority.  Refused -> 192 x 256 tile list */

/* ud_gemm_pick: one schedule code, plus the two flags for the large-tile instantiations */
#define UD_PICK_TILE128 0         /* 128-row tiles, 128 columns (plain 2-stage kernel) */
#define UD_PICK_TILE128_BN64 1    /*   64 columns (32 < N <= 64) */
#define UD_PICK_TILE128_BN32 2    /*   32 columns (N <= 32) */
#define UD_PICK_LIST192 3         /* 192 x 256 tile list */
#define UD_PICK_LIST256 4         /* 256 x 256 tile list */
#define UD_PICK_CONV_TILE 5       /* halo-tile 3x3 convolution (either head-conv kernel) */
#define UD_PICK_RING 6            /* 128 x 128 tiles, 4-stage pipelined ring */
#define UD_PICK_RING_SPLITK 7     /*   with the two-way K split across CUs */
#define UD_PICK_BALANCED 8        /* row-balanced schedule of the 256-column kernel */
#define UD_PICK_LIST192_SPLITK 10 /* 192 x 256 tiles with the two-way K split */
#define UD_PICK_PINGPONG 11       /* 192 x 256 tiles, ping-pong form */
#define UD_PICK_DUO 12            /* 192 x 128 tiles, two workgroups per CU */
#define UD_PICK_SCHEDULE 15       /* mask of the schedule code */
#define UD_PICK_LN_CONSUMER 16    /* flag: the folded-LayerNorm consumer instantiation runs (row_stats_in) */
#define UD_PICK_GROUPED 32        /* flag: a grouped problem runs as ONE large-tile launch */

typedef struct UdGemm {
  const void* A;
  const void* W;
  const float* bias;      /* [N] fp32 or NULL */
  void* out;
  void* out2;
  const float* add;       /* optional fp32 [*, ldadd] added before activation; row = (m % rows_in) + add_row_off */
  const void* zeros;      /* >= 256 B of zeros in device memory (padding source for conv A-modes) */
  const float* w2;        /* UD_EPI_HEAD: [N] second-layer (1x1 conv) weights */
  int M, N, K;            /* K = padded reduction length (multiple of 64) */
  int lda, ldw, ldc, ldc2, ldadd;
  int amode, epi, act, act2;
  int accumulate;         /* UD_EPI_F32: 0 = overwrite, 1 = out += result, 2 = result = out + acc but only the fp16 copy out2 is written */
  int rows_in, rows_out, row_off, add_row_off;   /* output row = (m / rows_in) * rows_out + (m % rows_in) + row_off; rows_in = 0 -> identity */
  /* conv A-modes: row m -> image m / rows_img, pixel p = m % rows_img (valid if p < Himg*Wimg) */
  int Himg, Wimg, Cin, cstride, coff, rows_img;
  long long img_stride;   /* elements between images of A */
  /* UD_EPI_QKV */
  int vsplit, tok_per_img, kv_ld, heads_v;
  /* UD_EPI_D2S: n = (a*k + c)*Co + o ; input row m -> image m / rows_in_img, p = m % rows_in_img -> (y, x) on [Hin, Win] */
  int d2s_k, d2s_Co, d2s_Hin, d2s_Win, d2s_rows_in_img;
  long long d2s_out_img_pix;   /* pixels between images in the output */
  /* UD_EPI_HEAD */
  float b2, post_add;
  /* groups: blockIdx.z = g offsets (elements) */
  int groups;
  long long gA, gW, gBias, gOut, gOut2, gW2;
  float b2_g1, post_add_g1;    /* group 1 constants for UD_EPI_HEAD */
  int tile_hint;               /* UD_HINT_* above: 0 = the cost model decides; the others force one schedule where it is eligible (tests, A/B tools) */
  /* optional scratch for the two-way K split of small problems (at most 128 tiles of 128x128, K >= 1024, dense A, F16 / F32
   * epilogues): two workgroups on different CUs each take half of K, the later one adds the other's fp32 partial tile (a + b is
   * order-independent, so results do not depend on timing) and runs the epilogue.  splitk_ws: 2 * tiles * 64 KB; splitk_cnt: one
   * unsigned per tile, zeroed ONCE by the caller (tickets are used by parity and never reset).  Both owned by the caller and not
   * shared between streams.  NULL = never split. */
  void* splitk_ws;
  void* splitk_cnt;
  int Hsrc, Wsrc;              /* UD_A_CONV3_REFLECT_UP: size of the low-resolution source image */
  /* Split-fp16 products by K concatenation (no second kernel): the reduction index may run PAST the stored width of one operand and
   * wraps around once.  Dense A: a_wrap = stored columns of A (multiple of 64), column k of the product reads A[:, k - a_wrap] for
   * k >= a_wrap; conv A-modes: a_wrap = stored channels per pixel (multiple of 8), `Cin` = channels the K index is decoded with
   * (e.g. 2 * a_wrap), channel c >= a_wrap reads channel c - a_wrap.  w_wrap: the same for W (dense A only).  0 = no wrap.
   * Use: W' = [W_hi | W_lo] (W_lo = fp16(W - W_hi), packed once at load time), K' = 2 K, a_wrap = K gives A W_hi^T + A W_lo^T = A W^T
   * with W exact to ~22 bits -- the weights' fp16 rounding is a SYSTEMATIC perturbation of the model (it shifts the predicted camera
   * and the log-depth of every pixel coherently; tools/v1_precision_study.py), unlike the activations' rounding which averages out.
   * Three terms [A_hi | A_lo | A_hi] x [W_hi | W_hi | W_lo] (a_wrap = 2 K) give an fp32-class product. */
  int a_wrap, w_wrap;
  /* LayerNorm folded into a producer / consumer pair of GEMMs (large-tile kernel, dense A; reference metadinov2/block.py:85-89 norm1 /
   * norm2 between `x += proj(..)` / `x += fc2(..)` and the following qkv / fc1 Linear): no second pass over the fp32 stream.
   *   producer (UD_EPI_F32): row_stats_out [M][N / 64][2] fp32 = (sum, sum of squares) of the STORED fp32 row values over every
   *     64-column slab (one entry per wave of the tile; fixed order: bit-reproducible); out2 = the raw fp16 copy of the row.
   *   ud_row_stats_finalize: [M][slabs][2] -> [M][2] = (rstd, -mean * rstd), slabs <= 16 summed in one fixed butterfly order -- or
   *     row_stats_final below: the same reduction inside the producer, no extra launch.
   *   consumer (UD_EPI_F16 / UD_EPI_QKV): A = the raw fp16 copy, row_stats_in = the finalized [M][2]; the epilogue stores
   *     act(rstd * acc - mean * rstd * wsum[n] + bias[n]), wsum[n] = sum_k W[n, k] over the fp16-ROUNDED weights (the LayerNorm's affine
   *     folded into W / bias as before): rstd (x - mean) W^T = rstd (x W^T - mean 1 W^T).  fp16(x) carries the same 2^-11 relative
   *     rounding as fp16(LN(x)) when |mean| <~ std, which holds for residual streams (tap tests).
   *   ln_D / ln_eps: read by the producer when row_stats_final is set; ln_slabs: unused by the kernels (kept for program recording). */
  float* max_out;              /* UD_EPI_F32, optional: fp32 [*, ldc] laid out like `out`; max_init != 0: max_out = stored value, else max_out =
                                * max(max_out, stored value) -- the running element-wise maximum over the block outputs of a ConvNeXt stage
                                * (utils/misc.py:18-21 max_stack, unidepthv1/decoder.py:366-373) taken where the value is produced instead of by
                                * a separate pass over the stream (ud_max_f32: 36 launches, 12 B per element) */
  int max_init;
  int grp_rows;                /* internal (callers leave 0): set by ud_gemm_f16 when it runs a grouped problem -- `groups` GEMMs stacked along M --
                                * as ONE tile list of the large-tile kernel: rows per group */
  float* row_stats_out;
  float* row_stats_final;      /* producer, optional: [M][2] = (rstd, -mean * rstd) written by the producer ITSELF -- the last workgroup to finish a row
                                * tile (one ticket per row tile in row_stats_ticket: ceil(M / 128) unsigned, zeroed ONCE by the caller, never reset)
                                * reduces the partial sums of all column tiles in ascending slab order; replaces ud_row_stats_finalize (a ~7.5 us
                                * launch).  Large-tile kernel, tile-list schedule, N <= 1024; uses ln_D / ln_eps. */
  unsigned* row_stats_ticket;
  const float* row_stats_in;
  const float* wsum;
  int ln_slabs, ln_D;
  float ln_eps;
  /* UD_EPI_D2S, optional (round 4): the value the transposed convolution accumulates INTO is not read from `out` but interpolated on the fly
   * from up_src -- fp32 NHWC [*, up_img_rows, up_ld] holding a (up_H x up_W) map per image -- as its bilinear x2 up-sampling
   * (align_corners=False: exactly ud_upsample2x_nhwc mode 0, upsample.py:184-186 nn.Upsample behind the 1x1 conv), so the up-sampled map is
   * never written and read back: out = up2(up_src) + ConvT(A) (+ bias), out2 = act2(out).  Needs d2s_Hin * d2s_k == 2 * up_H (same for W). */
  const float* up_src;
  int up_H, up_W, up_ld, up_img_rows;
  /* Round 6: two-way K split of the LARGE-tile list (192 x 256 tiles): a one-round list of 32..128 tiles with K >= 2048 (dense A or zero-padded
   * 3x3 taps, fp16 / fp32 epilogues without row statistics; the decoder's stage-0 residual-conv-unit convolutions, layers/upsample.py:137-163)
   * runs as 2 * tiles workgroups, each over one half of K; same exchange, same splitk_cnt parity tickets (one unsigned per tile, zeroed once)
   * as the small-tile split above.  Scratch: splitk_ws of splitk_ws_bytes >= 2 * tiles * 192 * 256 * 4 bytes; a smaller (or absent)
   * scratch keeps the unsplit schedules.  0 for callers that only provide the small-tile scratch. */
  long long splitk_ws_bytes;
} UdGemm;

int ud_gemm_f16(const UdGemm* desc, void* stream);
/* the schedule the call above runs this descriptor on, UD_PICK_* above (code + flags); host code only, nothing is launched */
int ud_gemm_pick(const UdGemm* desc);
/* kernel class of that schedule as rocprofv3 prints it, e.g. "gemm256_kernel<3, 1, 0, false, false, false, true, false>" (profiling labels:
 * profiles and bench lines join on it).  Writes at most cap bytes including the terminator; UD_ERR_BAD_ARG when the label does not fit. */
int ud_gemm_kernel_name(const UdGemm* desc, char* buf, int cap);

/* ---- LayerNorm (statistics only; the affine is folded into the consumer's weights at load time) ----
 * y(fp16)[orow, :] = (x[irow, :] - mean) * rsqrt(var + eps), biased variance (F.layer_norm).
 * Replaces nn.LayerNorm at metadinov2/block.py:85-89 (eps 1e-6, dinov2.py:167), dinov2.py:254,336-342 (eps 1e-5),
 * layers/attention.py:115-116, layers/mlp.py:29, decoder.py:186-188.
 * Row mapping: for r in [0, rows): img = r / rows_per_img, p = r % rows_per_img;
 *   irow = img * in_rows_per_img + p + in_row_off;  orow = img * out_rows_per_img + p + out_row_off. */
typedef struct UdLayerNorm {
  const float* x; void* y;
  int rows, D, ldx, ldy;
  float eps;
  int rows_per_img, in_rows_per_img, in_row_off, out_rows_per_img, out_row_off;
  int out_f32;            /* 0: y is fp16 (MFMA operand); 1: y is fp32 (the fp32 camera head) */
  const float* gamma;     /* optional affine [D] applied here (NULL = statistics only, the default: affines are folded into the consumer).  */
  const float* beta;      /* Needed where no linear consumer follows: the ConvNeXt stem's LayerNorm2d feeds a zero-padded depth-wise conv.  */
  const float* add;       /* optional fp32 [*, ldx] added to the input row BEFORE the statistics, indexed by the row's position inside its output
                           * image (out_row_off + p): `features + pos_embed` ahead of an MLP's norm (unidepthv1/decoder.py:80-83). */
  float* cls_y;           /* optional (round 6, fp16 output only): the launch covers rows_per_img + 1 rows per image (`rows` counts them); the FIRST of an */
  int ldcls;              /* image's rows -- input row in_row_off - 1, the class token in front of the patch tokens -- is normalised the same way and
                           * written as fp32 to cls_y[image * ldcls ..] (it feeds the fp32 camera head), the others as usual.  One launch instead of
                           * two per tapped layer of the encoder (dinov2.py:254 norm on x_norm_clstoken / x_norm_patchtokens). */
} UdLayerNorm;
int ud_layernorm_f32_f16(const UdLayerNorm* desc, void* stream);

/* partial (sum, sum of squares) pairs of UdGemm.row_stats_out [M][slabs][2] -> stats [M][2] = (rstd, -mean * rstd) with mean = S1 / D,
 * rstd = rsqrt(max(S2 / D - mean^2, 0) + eps) (biased variance, F.layer_norm): what UdGemm.row_stats_in consumes. */
int ud_row_stats_finalize(const float* partials, float* stats, int M, int slabs, int D, float eps, void* stream);

/* ---- fp32 small-M linear layer (camera head only) ---------------------------------------------------------
 * out[m, n] (+)= act(sum_k x[m,k] W[n,k] + bias[n] + add[m % add_mod, n]),  everything fp32, exact-erf GELU.
 * The camera head (decoder.py:48-114) maps 4 tokens per image to the pinhole parameters that generate EVERY ray; its
 * rounding error is amplified by the 2^k*pi ray-angle bands (decoder.py:246-252) into a common-mode depth error, so it is
 * the one place where fp16 MFMA operands are not accurate enough (measured: K error 1e-3 -> depth ARel 1e-3) and, at
 * M = 4*B rows, the one place where fp32 costs nothing.  Replaces nn.Linear in CameraHead / camera_token_adapter. */
typedef struct UdLinearF32 {
  const float* x; const float* W; const float* bias; const float* add; float* out;
  int M, N, K, ldx, ldw, ldc, ldadd, add_mod;
  int act, accumulate;
} UdLinearF32;
int ud_linear_f32(const UdLinearF32* desc, void* stream);

/* fp32 attention over T <= 8 tokens per image (camera head, layers/attention.py:81-165 with 4 tokens):
 * q [B*T, C], kv [B*T, 2C] = [K | V] heads-major, out [B*T, C]; H heads of width C/H. */
int ud_attention_small_f32(const float* q, const float* kv, float* out, int B, int T, int H, int C, float scale, void* stream);

/* ---- the whole camera head as ONE launch ------------------------------------------------------------------------
 * CameraHead.forward (decoder.py:94-108: project MLP, two AttentionBlocks over the 4 camera tokens of an image, out_pinhole MLP) and the four
 * camera_token_adapter Linears in front of it (decoder.py:34-45, 418-433) are ~26 dependent launches of the two fp32 kernels above, each a few
 * microseconds of work behind ~10 us of launch and fill latency (0.38 ms per infer() at bs = 8, 7 % of a bs = 1 call).  Here the chain is a
 * list of PHASES run by one persistent grid: phase = [LayerNorm of the input rows] -> out (+)= act(x W^T + bias + add) over a column slice per
 * workgroup, or the T-token attention per (image, head); workgroups meet at a grid barrier (one agent-scope counter) where a phase reads what
 * the previous one wrote.  Activations cross XCDs with system-scope (sc0 sc1) stores and loads -- the L2s of the 8 XCDs are not coherent with each
 * other inside a kernel -- while the next phase's weight slab streams into LDS under the barrier.  Same arithmetic as the launches it replaces
 * (fp32 FMA chains, two-pass LayerNorm, erf GELU); the summation order over k differs (32 interleaved slices per row, then a butterfly).
 * Limits (ud_camera_head_f32 returns UD_ERR_UNSUPPORTED otherwise and the caller keeps the per-layer launches): linear phases need K % 128 == 0,
 * ceil(N / workgroups) * K * 4 <= 32 KB, LayerNorm phases K <= 512; attention T <= 8, C / H <= 64; n_phases <= UD_CAM_MAX_PHASES. */
#define UD_CAM_MAX_PHASES 24
typedef struct UdCamPhase {
  const float* x;        /* linear: input rows [M, K] (ldx).  attention: packed rows [q | k | v] (ldx), q at column 0, k at C, v at 2 C */
  const float* W;        /* [N, K] row-major, dense (row stride K) */
  const float* bias;     /* [N] or NULL */
  const float* add;      /* [add_mod, ldadd] or NULL: out[m, n] += add[m % add_mod, n] for n < add_cols (latents_pos on the q columns) */
  float* out;            /* [M, N] (ldc) */
  int M, N, K, ldx, ldc, ldadd, add_mod, add_cols;
  int kind;              /* 0 linear, 1 attention */
  int ln;                /* 1: the input rows are layer-normalised first (statistics only: the affine is folded into W / bias by the caller) */
  int act, accumulate;   /* UD_ACT_NONE / UD_ACT_GELU; accumulate: out += ... */
  int sync;              /* 1: grid barrier after this phase (the next phase reads what this one wrote) */
} UdCamPhase;
typedef struct UdCameraHead {
  UdCamPhase ph[UD_CAM_MAX_PHASES];
  int n_phases;
  int T, H, C;           /* attention phases: tokens per image, heads, width (head width C / H) */
  float scale, eps;      /* softmax scale; LayerNorm eps */
  unsigned* sync_ws;     /* 16 words, zero before the FIRST launch; every launch leaves words 0 and 1 zero again.  Word 2 != 0 afterwards: a
                          * grid barrier timed out (the grid was not co-resident: CU mask, partitioned device, foreign kernels holding CUs).
                          * The failure is LOUD: every launch that ends with word 2 set overwrites the LAST phase's output (the camera
                          * parameters) with NaN, so intrinsics, rays and depth of that call are NaN; word 2 stays set (and keeps poisoning)
                          * until the caller clears it */
  int workgroups;        /* 0 = default (128) */
  unsigned* fail_host;   /* optional, HOST-mapped (pinned) word: set to 1 together with word 2 by a system-scope store, so the caller can poll
                          * the failure without a device synchronisation (unidepth_amd checks it at the start of the next infer()) */
  unsigned spin_limit;   /* polls of a barrier before a workgroup gives up; 0 = default (2^22: seconds).  Tests force the time-out with 1 */
} UdCameraHead;
/* Launches of ud_camera_head_f32 on one device are SERIALISED across streams (an event chain inside the library: the next launch waits for the
 * previous one wherever it was enqueued), so two spinning grids of one process are never resident together. */
int ud_camera_head_f32(const UdCameraHead* desc, void* stream);
int ud_camera_head_supported(const UdCameraHead* desc);   /* UD_OK if ud_camera_head_f32 would take this descriptor (host-side check, nothing is launched) */

/* ---- fused multi-head attention forward, head_dim 64 (padded), no mask, fp16 in/out, fp32 softmax ----
 * O = softmax(Q K^T * scale) V per (image, head).  Replaces F.scaled_dot_product_attention at
 * metadinov2/attention.py:58 and layers/attention.py:136-138 (and xformers memory_efficient_attention :77).
 * Q [img*q_rows_per_img + i, h*64 + d] (ldq), K likewise (ldk), Vt = V^T [img][h][64][kv_ld] in the UD_EPI_QKV block order
 * (zeros beyond Nk up to the next multiple of 64), O like Q (ldo).
 * kv_broadcast != 0: groups of kv_group consecutive images share one K/V image (single GT camera, decoder.py:400). */
typedef struct UdAttention {
  const void* Q; const void* K; const void* Vt; void* O;
  int B, H, Nq, Nk;
  int ldq, ldk, ldo, kv_ld;
  int q_rows_per_img, k_rows_per_img;
  float scale;
  int kv_broadcast;
  int kv_group;           /* with kv_broadcast: image i uses the K/V of image i / kv_group (0 -> all share image 0) */
  int q_prescaled;        /* != 0: Q already holds q * scale * log2(e) (folded into the q projection by the caller): `scale` is ignored and the
                           * kernel skips the per-score multiply (softmax(q k^T scale) is unchanged) */
} UdAttention;
int ud_attention_f16(const UdAttention* desc, void* stream);

/* ---- pre-processing + im2col for the 14x14 patch embedding ---------------------------------------------
 * Replaces unidepthv2.py:288-297 (/255, ImageNet mean/std, zero pad, bilinear align_corners=False resize) and
 * the unfold implied by Conv2d(k=s=14) (patch_embed.py:71-88).  rgb: uint8 (is_u8) or fp32 [B,3,H,W].
 * patches(fp16)[img*hw + py*w + px, c*196 + i*14 + j], row stride ldp (>= 588, pad cols untouched). */
typedef struct UdPreprocess {
  const void* rgb; void* patches;
  int B, H, W;            /* source image */
  int pad_l, pad_t, Hp, Wp;   /* padded size (before resize) */
  int Hn, Wn;             /* network input size (multiples of 14) */
  int ldp;
  int is_u8, normalize;
  float mean[3], inv_std[3];
} UdPreprocess;
int ud_preprocess_patches(const UdPreprocess* desc, void* stream);

/* ---- small helpers ----------------------------------------------------------------------------------- */
/* dst(fp32)[img*rows_per_img + row_off, :D] = src[:D]  (cls token + pos_embed[0]; dinov2.py:316-317) */
int ud_fill_rows_f32(float* dst, const float* src, int n_img, int rows_per_img, int row_off, int D, int ld, void* stream);

/* camera head tail (decoder.py:85-99 fill_intrinsics, :361-403 run_camera; unidepthv2.py:92-108 _postprocess_intrinsics):
 * raw[(b*4 + j) * raw_stride] = j-th raw camera parameter of image b -> intr4 [B,4] = (fx,fy,cx,cy) at network
 * resolution, K33 [B,9] row-major, Kinv33 [B,9] (closed-form pinhole inverse), Kpost33 [B,9] = K with
 * fx,fy,cx,cy /= resize_factor and cx -= pad_l, cy -= pad_t (the matrix infer() returns). */
int ud_camera_intrinsics(const float* raw, int raw_stride, float* intr4, float* K33, float* Kinv33, float* Kpost33,
                         int B, int Hn, int Wn, float resize_factor, int pad_l, int pad_t, void* stream);

/* rays [nb,3,Hn,Wn] fp32 = normalise(Kinv @ [u+0.5, v+0.5, 1]) (utils/coordinate.py:4-20 pixel centres).
 * gt_mode 0: predicted camera, norm clamp 1e-5 (decoder.py:389-393);
 * gt_mode 1: user camera (utils/camera.py:254-266 Pinhole.unproject: divide by z.clip(1e-4); :88-92 norm clamp 1e-4).
 * gt_mode 2 / 3: user EUCM / Spherical camera (utils/camera.py:307-328 / :371-386 unproject + :88-92 get_rays); the 9 floats per
 *   camera are then the model parameters at network resolution: (fx, fy, cx, cy, alpha, beta, -, -, -) resp.
 *   (fx, fy, cx, cy, width, height, hfov/2, vfov/2, -) instead of an inverse intrinsic matrix. */
int ud_rays_from_kinv(const float* Kinv33, float* rays, int nb, int Hn, int Wn, int gt_mode, void* stream);

/* rays [1,3,Hn,Wn] fp32 of ONE user camera whose unprojection is iterative (utils/camera.py get_rays :88-92 over
 * OPENCV.unproject :496-694 (model 4), Fisheye624.unproject :778-974 (model 5), MEI.unproject :985-1082 (model 6)).
 * params: device pointer, 16 floats [fx, fy, cx, cy, k1..k6, p1, p2, s1..s4] (models 4, 5; OPENCV: k4..k6 = 0) or 9 floats
 * [fx, fy, cx, cy, k1, k2, p1, p2, xi] (model 6), at network resolution.  Which distortion groups are active is decided on
 * the device from the parameters, like the reference's use_radial / use_tangential / use_thin_prism.
 * scratch: 4*Hn*Wn + 16 floats (models 4, 5; may be NULL for MEI) -- per-pixel solver state plus the per-iteration maximum
 * residual that reproduces the reference's image-wide early exit of the radial trust-region loop (:629-631). */
int ud_rays_from_camera(const float* params, float* rays, float* scratch, int Hn, int Wn, int model, void* stream);

/* ray embedding (decoder.py:234-253): antialiased bilinear down-sample of rays [nb,3,Hn,Wn] to (h,w)
 * (utils/geometric.py:227-252), renormalise (clip 1e-4), polar/azimuth, C/2 log-spaced sine bands each
 * (utils/positional_embedding.py:218-256; `scales` = the C/2 band frequencies, fp32), then LayerNorm statistics
 * (eps) -> xhat fp16 [img*rows_per_img + token, ldy]. */
typedef struct UdRayEmbed {
  const float* rays; const float* scales; void* xhat;
  int nb, Hn, Wn, h, w, C, ldy, rows_per_img;
  float eps;
} UdRayEmbed;
int ud_ray_embed(const UdRayEmbed* desc, void* stream);

/* x2 bilinear up-sampling, align_corners=False (nn.Upsample in layers/upsample.py:215-217), NHWC fp32 in [B,H,W,C] (row stride ldin).
 * mode 0: out fp32 [B,2H,2W,C]; mode 1: out = LayerNorm-statistics(fp16) of the up-sampled pixel (eps), row stride ldy. */
typedef struct UdUpsample2x {
  const void* in; void* out;
  int B, H, W, C, ldin, ldy, mode;
  float eps;
  int in_img_rows;   /* rows (pixels) between consecutive images of `in`; 0 -> H*W */
} UdUpsample2x;
int ud_upsample2x_nhwc(const UdUpsample2x* desc, void* stream);

/* bilinear resize, align_corners=True (decoder.py:299-301,309-311), NHWC fp16 -> NHWC fp16, G groups */
typedef struct UdResizeAC {
  const void* in; void* out;
  int G, B, Hin, Win, Hout, Wout, C;
} UdResizeAC;
int ud_resize_ac_nhwc_f16(const UdResizeAC* desc, void* stream);

/* output assembly (decoder.py:456-462, unidepthv2.py:375-377, :310-339): fp32 NCHW resize (F.interpolate align_corners=False,
 * bilinear or bicubic = the two modes the reference's `interpolation_mode` accepts) + crop of _postprocess (unidepthv2.py:80-89). */
typedef struct UdFinalize {
  const float* radius_net;  /* [B,Hn,Wn] */
  const float* conf_net;    /* [B,Hn,Wn] */
  const float* rays_net;    /* [nb_rays,3,Hn,Wn] */
  float* confidence; float* radius; float* depth; float* points; float* rays;   /* outputs at [.,.,Ho,Wo] */
  int B, nb_rays, Hn, Wn;
  int Hp, Wp;               /* padded (pre-crop) size the network maps are resized to */
  int pad_l, pad_t, Ho, Wo; /* crop */
  int mode;                 /* resampling of _postprocess (unidepthv2.py:80-89, `interpolation_mode`): 0 bilinear, 1 bicubic; align_corners=False */
} UdFinalize;
int ud_finalize_outputs(const UdFinalize* desc, void* stream);

/* NHWC fp32 (row stride ld, rows_per_img rows per image) -> NCHW fp32 [B,C,h*w]  (depth_features, decoder.py:265-267) */
int ud_nhwc_to_nchw_f32(const float* in, float* out, int B, int hw, int C, int ld, int rows_per_img, void* stream);

/* ---- ConvNeXt-side ops of the UniDepthV1 path (reference backbones/convnext.py; decoder blocks layers/convnext.py) ---------------
 * Depth-wise 7x7 convolution, zero padding 3 (convnext.py:171-179 conv_dw via timm create_conv2d(depthwise=True); layers/convnext.py:16-24):
 * y[b,y,x,c] = bias[c] + sum_{ky,kx} w[(ky*7+kx)*C + c] * x[b, y+ky-3, x+kx-3, c];  NHWC fp32 in / out, pixel strides ldx / ldy (floats);
 * w is TAP-major [49][C] (repacked from the reference's [C,1,7,7] at load time). */
typedef struct UdDwConv7 {
  const float* x; const float* w; const float* bias; float* y;
  int B, H, W, C, ldx, ldy;
  /* Round 6 (VERDICT r5 missing #5c), the LayerNorm behind the convolution (convnext.py:215-216 `x = self.norm(x)`) folded into the producer / consumer pair:
   * y16 (optional; then y may be NULL): the convolution's output as RAW fp16 [pixels, ldy16] -- the A operand of a LayerNorm-folded consumer GEMM
   * (UdGemm.row_stats_in); stats_out (with y16): per pixel and 64-channel slab the (sum, sum of squares) of the fp32 outputs, [pixels][C / 64][2] =
   * UdGemm.row_stats_out's layout, reduced by ud_row_stats_finalize (C / 64 <= 16).  C % 64 == 0 (the LDS-tiled kernel). */
  void* y16; float* stats_out; int ldy16;
  /* optional, with stats_out: the LAST of a pixel tile's C / 64 channel blocks to finish (one ticket per 8 x 16 tile of output pixels: stats_ticket, >= number of
   * tiles unsigned words, zeroed once by the caller, self-resetting) reduces the tile's partial sums in slab order and writes stats_final [pixels][2] =
   * (rstd, -mean * rstd) with eps ln_eps -- what ud_row_stats_finalize would write; no reduction launch. */
  float* stats_final; unsigned* stats_ticket; float ln_eps;
} UdDwConv7;
int ud_dwconv7_nhwc_f32(const UdDwConv7* desc, void* stream);
/* LayerNorm2d statistics (eps; affine folded into the conv weights) of every pixel of x fp32 NHWC [B,H,W,C], written as fp16 into the
 * im2col image of the following Conv2d(k=2, s=2, pad 0) (convnext.py:245-266 ConvNeXtStage.downsample): row (b, y/2, x/2), columns
 * ((y&1)*2 + (x&1))*C + c, row stride ldo >= 4C; an odd last row / column of x is dropped like the convolution drops it. */
int ud_layernorm_patchify2(const float* x, void* out, int B, int H, int W, int C, int ldo, float eps, void* stream);
/* im2col of the 4x4 stride-4 stem convolution (convnext.py:370-383): img fp32 NCHW [B,3,H,W] -> fp16 [B*(H/4)*(W/4), ldo], column
 * c*16 + ky*4 + kx (48 used; the caller zero-fills the pad columns once). */
int ud_patchify4_nchw(const float* img, void* out, int B, int H, int W, int ldo, void* stream);
/* dst = init ? src : max(dst, src), element-wise over n fp32 values (utils/misc.py:18-21 max_stack over a stage's block outputs). */
int ud_max_f32(float* dst, const float* src, long long n, int init, void* stream);
/* out[b*ldo + c] = mean over the HW pixels of x[b, :, c] (x fp32 [B,HW,C]): the "class tokens" of the ConvNeXt wrapper (convnext.py:458). */
int ud_spatial_mean_f32(const float* x, float* out, int B, int HW, int C, int ldo, void* stream);

/* ---- decoder-side ops of the UniDepthV1 path that are not GEMMs / attention / LayerNorm: one entry point, dispatched on `kind` ----
 * a, b, c: inputs; out, out2: outputs (c is an output for UD_V1_CAMERA); i[], f[]: per-kind integers / floats as listed.
 *  RESIZE_AA     F.interpolate(bilinear, align_corners=False, antialias=True) of a crop window of an NHWC fp32 map (utils/geometric.py:227-252
 *                flat_interpolate; unidepthv1.py:66-86 _postprocess).  i = B, Hi, Wi, Ho, Wo, C, ldi, ldo, y0, x0, Hc, Wc (C % 4 == 0)
 *  SH_EMBED      rays [nb,3,Hn,Wn] -> antialiased resize to (h, w), F.normalize, 81 real spherical harmonics (utils/sht.py:833 rsh_cart_8),
 *                LayerNorm statistics (eps f[0]) -> fp16 [nb*rows_per_img, ldo >= 128] (decoder.py:205-222).  i = nb, Hn, Wn, h, w, ldo, rows_per_img
 *  SOFTMAX       out[r, :N] = softmax(f[0] * a[r, :N]) rows of fp32 scores -> fp16 (or fp32), pad columns N..ldo zero (the softmax inside
 *                F.scaled_dot_product_attention for single-head width-512 attention, layers/attention.py:136).
 *                i = rows & 0x7fffffff, N, ldi, ldo, out_f32, rows >> 31
 *  ATTN_FEWQ     T <= 8 queries against Nk keys, ONE head of width D (camera head `aggregate`, decoder.py:94, layers/attention.py:81-165):
 *                a = q fp32 [B*T, D], b = kv fp16 [B*Nk, 2D] = [K | V], out fp32 [B*T, D].  i = B, T, Nk, D; f[0] = scale
 *                c (optional) = fp32 scratch of B * ceil(Nk / 64) * T * (D + 2) floats: the keys are then processed in chunks of 64 by
 *                separate workgroups and merged in a second launch (deterministic order)
 *  HEAD_MIX      the attention of layers_8 / layers_4 AS THE REFERENCE COMPUTES IT (layers/nystrom_attention.py:59-62,81: q, k, v go to xformers
 *                NystromAttention as [b, n, h, d]; its `seq_len = k.size(-2)` is then h <= num_landmarks, so it takes its plain-softmax branch
 *                over the last two axes): per token, softmax((q_i / sqrt d) . k_j over the h heads j) v_j.  a = q fp32 [M, ldq], b = [K | V] fp32
 *                [M, ldkv], out fp16 [M, ldo]; head width 64.  i = M, h (2 / 4 / 8), ldq, ldkv, ldo; f[0] = 1 / sqrt(d)
 *  ADD           out = a + b (fp32; latents + ray embedding, decoder.py:263,283,303).  i = n & 0x7fffffff, n >> 31
 *  COPY_ROWS     out[(img*rows_per_img + row_off + t)*ld + d] = a[(img*T + t)*D + d] (torch.cat of token groups).  i = n_img, T, rows_per_img, row_off, D, ld, to_f16
 *                to_f16 == 2 (ld >= 2 D): the value as TWO fp16 terms, hi at column d and lo = fp16(x - hi) at column D + d -- the A operand
 *                [A_hi | A_lo] of a three-term product against [W_hi | W_hi | W_lo] (UdGemm.a_wrap = 2 K)
 *  RESIZE_AC_SPLIT  nn.UpsamplingBilinear2d (align_corners=True, layers/upsample.py:34) of an fp32 NHWC map, written as [hi | lo] fp16
 *                (2 C channels per pixel) for the 3x3 convolution behind it.  i = B, Hin, Win, Hout, Wout, C (C % 4 == 0)
 *  CAMERA        raw [B*4] -> K33 (out), its inverse (out2), post-processed K (c) (decoder.py:85-99,347-353; unidepthv1.py:88-92).
 *                i = B, Hn, Wn, pad_l, pad_t; f[0] = ratio
 *  POINTS        z map + K33 -> points [B,3,H,W] (out), depth [B,1,H,W] (out2) (unidepthv1.py:353-371; utils/geometric.py:45-73).  i = B, H, W, ldz, nK
 *  MEAN3         out = (a + b + c) / 3 on column 0 of strided maps (unidepthv1.py:66-77).  i = n & 0x7fffffff, ld, n >> 31
 *  VIT_TAP       UniDepthV1 on a DINOv2 backbone: out = init ? v : max(out, v), v = patch tokens + class token of the block whose residual
 *                stream is a [B*Np, D] (row 0 of an image = class token): unidepthv1.py:324-328 + decoder.py:366-373 max_stack; out2
 *                (optional) = the raw class tokens [B, D].  i = B, Np, hw, D, init
 *  OUT_CONV3     out[pixel, 0] = exp(clamp(conv3x3(x)[pixel] + f[0], -10, 10)) for ONE output channel, zero padding, everything fp32: the multi-scale
 *                outputs out8 / out4 / out2 (unidepthv1/decoder.py:185-187 nn.Conv2d(C, 1, 3, padding = 1), :250-298).  a = x NHWC [B, H, W, C],
 *                b = w [9, C] (tap = ky * 3 + kx), out [B * H * W, ldo].  i = B, H, W, C (% 4 == 0), ldo
 *  PREPROCESS    V1 network image (unidepthv1.py:305-321,50-56): [/255], ImageNet normalise, antialiased resize to (h, w), zero pad to (Hn, Wn).
 *                i = B, H, W, h, w, Hn, Wn, pad_l, pad_t, is_u8, div255, normalize */
enum { UD_V1_RESIZE_AA = 1, UD_V1_SH_EMBED = 2, UD_V1_SOFTMAX = 3, UD_V1_ATTN_FEWQ = 4, UD_V1_HEAD_MIX = 5, UD_V1_ADD = 8, UD_V1_COPY_ROWS = 9,
       UD_V1_CAMERA = 11, UD_V1_POINTS = 12, UD_V1_MEAN3 = 13, UD_V1_PREPROCESS = 14, UD_V1_VIT_TAP = 15, UD_V1_RESIZE_AC_SPLIT = 17, UD_V1_OUT_CONV3 = 18 };
typedef struct UdV1Op {
  int kind;
  const void* a; const void* b; void* c; void* out; void* out2;
  int i[12];
  float f[4];
} UdV1Op;
int ud_v1_op(const UdV1Op* desc, void* stream);

/* ---- the exchange step of batch data parallelism: all-gather of the packed output rows over RCCL / xGMI ----
 * The reference has no distributed inference path (unidepth/utils/distributed.py:153-176 sync_tensor_across_gpus is its pad -> gather -> trim
 * helper for variable-length gathers; unidepth_amd/dist.py keeps that pattern on the host).  One process per GPU, one communicator per
 * process; librccl is opened on first use.  Rank 0 calls ud_rccl_unique_id and hands the 128 bytes to the other ranks by any host channel;
 * every rank then calls ud_rccl_init with the calling thread's HIP device set.
 *   ud_rccl_allgather_outputs: recv [world][bytes_per_rank] <- every rank's `send` [bytes_per_rank] (device buffers, equal size on all ranks),
 *   enqueued on `stream`; direct != 0: the all-pairs send / receive group (every peer over its own xGMI link) instead of ncclAllGather. */
int ud_rccl_unique_id(void* id128);
int ud_rccl_init(const void* id128, int world, int rank);
int ud_rccl_allgather_outputs(const void* send, void* recv, size_t bytes_per_rank, int direct, void* stream);
int ud_rccl_finalize(void);

/* ---- the reference's two native extensions (evaluation / loss side), forward only ----
 * K nearest neighbours of every p1 point among the p2 points of the same cloud: replaces KNN.knn_points_idx
 * (unidepth/ops/knn/src/knn_ext.cpp:8 -> knn.h:44-80 KNearestNeighborIdx -> knn.cu:314-419 KNearestNeighborIdxCuda; caller
 * functions/knn.py:72 _knn_points.forward <- utils/chamfer_distance.py:143-144 <- utils/evaluation_depth.py:12-34).
 *   p1 [N,P1,D], p2 [N,P2,D] fp32 contiguous; lengths1/lengths2 int64 [N] or NULL (= P1 / P2 everywhere).
 *   dists fp32 [N,P1,K] squared L2 (norm 2) or L1 (norm 1) distances, idx int64 [N,P1,K]; every element is written (padding = 0).
 *   The K neighbours are the K smallest (dist, index) pairs in ascending order, i.e. already what functions/knn.py:75-91 obtains by
 *   sorting; ties resolve to the lower index (knn_cpu.cpp:40-58).  1 <= D <= 32 (D <= 8 on the register path), 1 <= K <= 32.
 *   A slot whose distance is +inf (an inf coordinate, a square that overflows) reports index 0, with or without the P2 split.
 *   work: optional u64 [N*P1] scratch; when given and K == 1, small P1 problems are split over P2 (ud_knn_split slices). */
typedef struct UdKnn {
  const float* p1; const float* p2;
  const long long* lengths1; const long long* lengths2;
  float* dists; long long* idx;
  unsigned long long* work;
  int N, P1, P2, D, K, norm;
} UdKnn;
int ud_knn_points(const UdKnn* desc, void* stream);
int ud_knn_split(const UdKnn* desc);
/* Patch gather: replaces RandomPatchExtraction.extract_patches_forward (unidepth/ops/extract_patches/src/extract_patches.cpp:3-6 ->
 * src/cuda/extract_patches_kernel.cu:9-35,65-95) together with the zero padding its module does first (modules/patch_extractor.py:26-42).
 *   in fp32 [B,C,H,W]; centers int32 [B,N,2] = (y, x) in the coordinates of the image padded by (pad_h, pad_w) on every side (pass
 *   pad = 0 for raw coordinates); out fp32, B*N*C*h*w elements in [b][n][c][i][j] order -- the order the reference kernel writes
 *   (extract_patches_kernel.cu:91), which it then views as {B,C,N,h,w} (:22).  Pixels outside the image read as 0. */
typedef struct UdExtractPatches {
  const float* in; float* out; const int* centers;
  int B, C, H, W, N, h, w, pad_h, pad_w;
} UdExtractPatches;
int ud_extract_patches(const UdExtractPatches* desc, void* stream);
/* 2-D depth metrics of a batch: replaces utils/evaluation_depth.py eval_depth (its DICT_METRICS applied per image after the bilinear
 * resample of the predictions), as a few stream-ordered launches with no host synchronisation (csrc/evaldepth.hip).
 *   gt fp32 [B,H,W]; pred fp32 [B,h,w] (bilinear align_corners=False to H x W, source index clamped at 0; identity when h = H and w = W);
 *   mask u8 [B,H,W] (nonzero = valid) or NULL (every pixel valid); has_max_depth != 0 also drops pixels with !(g <= max_depth).
 *   thresholds fp32 [200]: the 100 d_auc thresholds 1.25^e_k (non-decreasing), then the 100 exponents e_k (the trapezoid abscissae).
 *   out fp32 [18,B] in the reference's key order: d1_ssi d1_si d1 d2 d3 rmse rmselog arel_ssi arel_si arel sqrel log10 silog medianlog
 *   d_auc tau_ssi tau_si tau; an image with no valid pixel gives NaN in every row.
 *   work: device scratch of at least ud_eval_depth_work_bytes(B, H, W) bytes (host-only query), work_bytes its size.
 *   Bitwise reproducible: fp64 sums reduced in a fixed order, integer atomics only. */
typedef struct UdEvalDepth {
  const float* gt; const float* pred; const unsigned char* mask; const float* thresholds;
  float* out; void* work;
  int B, H, W, h, w;
  float max_depth; int has_max_depth;
  long long work_bytes;
} UdEvalDepth;
int ud_eval_depth(const UdEvalDepth* desc, void* stream);
long long ud_eval_depth_work_bytes(int B, int H, int W);
/* 3-D point metrics of a batch: replaces utils/evaluation_depth.py eval_3d (:160-182: the nearest-exact resample to about 240 x 320 valid
 * points per batch, then per image DICT_METRICS_3D = MSE_3d, chamfer, F1 on the masked points), as eight stream-ordered launches with no
 * host synchronisation and no device-to-host copy (csrc/eval3d.hip).
 *   gt, pred fp32 [B,3,H,W]; mask u8 [B,H,W] (nonzero = valid); thresholds fp32 [T], compared with SQUARED distances, any order.
 *   Sample size, on the device from S = the number of valid pixels of the batch, in the reference's fp32 arithmetic:
 *   q = 76800.0f / (float)S, r = sqrtf(q) correctly rounded; r >= 1: (h, w) = (H, W); else h = (int)((float)H * r), w = (int)((float)W * r).
 *   gt, pred and mask are sampled on the h x w grid by F.interpolate(mode="nearest-exact")'s rule, source = min(floor((dst + 0.5f) *
 *   ((float)in / (float)out)), in - 1); the valid samples of image b, row-major, are its n_b points (the order of gt[:, mask]).
 *   S = 0, h = 0 or w = 0: every image is empty (size still reports the rule's (h, w); S = 0 reports (H, W)).
 *   out fp32 [3,B], rows MSE_3d, chamfer, F1 of every image:
 *     MSE_3d   mean over the points of the fp32 L2 norm of gt - pred;
 *     chamfer  mean of (sqrtf(d1_i) + sqrtf(d2_i)) / 2, d1 = gt -> pred and d2 = pred -> gt the squared distances to the nearest
 *              neighbour, bit-equal to ud_knn_points' dists on the same rows (K = 1, norm 2);
 *     F1       c1_t = #(d1 < th_t), c2_t = #(d2 < th_t) (strict, fp32); p_t = (float)c1_t / (float)n_b, r_t = (float)c2_t / (float)n_b,
 *              f_t = 2 p_t r_t / (p_t + r_t) in fp32 with NaN -> 0; F1 = trapz(f, dx = 1) / T (0 for T = 1);
 *     an image with n_b = 0 gets NaN in all three rows (the reference skips it and returns fewer rows: out[:, counts > 0] is its result).
 *   counts int64 [B] = n_b; size int32 [2] = (h, w).
 *   work: device scratch, 16-byte aligned, of at least ud_eval_3d_work_bytes(B, H, W, T) bytes (host-only query; -1 for sizes outside the
 *   limits), work_bytes its size.  It is sized for H * W points per image: no tighter bound is known on the host.
 *   Limits: 1 <= B <= UD_EVAL3D_MAX_B, H, W >= 1, H * W < 2^31 - 1024, B * H * W < 2^36 (launch grids), 1 <= T <= UD_EVAL3D_MAX_T (the
 *   thresholds and their counters sit in LDS; the reference uses 100).
 *   Bitwise reproducible: fp64 sums reduced in a fixed order, integer atomics only. */
#define UD_EVAL3D_MAX_B 32767
#define UD_EVAL3D_MAX_T 1024
typedef struct UdEval3d {
  const float* gt; const float* pred; const unsigned char* mask; const float* thresholds;
  float* out; long long* counts; int* size;
  void* work; long long work_bytes;
  int B, H, W, T;
} UdEval3d;
int ud_eval_3d(const UdEval3d* desc, void* stream);
long long ud_eval_3d_work_bytes(int B, int H, int W, int T);
/* Ground-truth point maps of a batch: the device form of Camera.reconstruct (utils/camera.py; datasets/base_dataset.py add_points),
 * one camera model per image, stream-ordered, no host synchronisation (csrc/reconstruct.hip).
 *   depth fp32 [B,1,H,W]; params fp32 [B,16] on the device, rows zero-padded, layouts as in csrc/camera_models.h (Pinhole fx fy cx cy;
 *   EUCM + alpha beta; Spherical + W H hfov/2 vfov/2); model[b] = 1 Pinhole, 2 EUCM, 3 Spherical, 4 OPENCV, 5 Fisheye624, 6 MEI.
 *   points fp32 [B,3,H,W].  Pixel centres are u + 0.5, v + 0.5; every maximum lets a NaN through (`x < m ? m : x`):
 *     Pinhole     r = K^-1 [u, v, 1] = ((u - cx) / fx, (v - cy) / fy, 1), no skew;  r / max(r.z, 1e-4) * max(depth, 0)
 *     Spherical   the unit-sphere direction, re-normalised with the 1e-5 floor, * depth (no clamp: a negative depth passes through)
 *     EUCM        r = (c mx, c my, max(c mz, 1e-3));                              r / max(r.z, 1e-4) * max(depth, 1e-4)
 *     OPENCV, Fisheye624   r = (dx, dy, 1) of the solvers, not normalised;        same formula
 *     MEI         r = (dx, dy, pz), not normalised (pz <= 0 at wide angles: the 1e-4 floor decides);  same formula
 *   A batch without an OPENCV / Fisheye624 member is one launch.  With n_iterative > 0 such members: one init launch (it also does every
 *   closed-form image), 10 trust-region step launches over the iterative images only, one final launch, whatever B is.  Every iterative
 *   image leaves the radial loop on its own, once ITS largest |residual| is below 1e-3 (the reference runs each member of a BatchCamera
 *   separately); the maxima are cleared by the call (a memset node on `stream`), so a captured graph can be replayed.
 *   work: device scratch, 16-byte aligned, of at least ud_reconstruct_work_bytes(B, H, W, n_iterative) bytes (host-only query; -1 for
 *   sizes outside the limits; 0 and work may be NULL when n_iterative = 0): 11 maxima and a float4 solver state per pixel of every
 *   iterative image.  Limits: 1 <= B <= UD_RECON_MAX_B, H, W >= 1, H * W < 2^31 - 256.  Built with -ffp-contract=off: every operation
 *   rounds separately. */
#define UD_RECON_MAX_B 256
typedef struct UdReconstruct {
  const float* depth; const float* params; float* points;
  void* work; long long work_bytes;
  int B, H, W;
  unsigned char model[UD_RECON_MAX_B];
} UdReconstruct;
int ud_reconstruct(const UdReconstruct* desc, void* stream);
long long ud_reconstruct_work_bytes(int B, int H, int W, int n_iterative);

/* The other direction: the points of a batch projected to image coordinates, the device form of Camera.project (utils/camera.py:
 * Pinhole :239-252, EUCM :281-304, Spherical :359-368, OPENCV :423-493, Fisheye624 :705-775, MEI :1084-1142, BatchCamera :1158-1164),
 * one camera model per image, in ONE launch with one thread per point (csrc/project.hip; the arithmetic is csrc/camera_models.h
 * ud_cam_project_<model>).  Stream-ordered, no host synchronisation, no work buffer.
 *   xyz fp32: coordinate c of point r of image b is at xyz[b * batch_stride + r * point_stride + c * comp_stride] (ELEMENTS), as UdSplat:
 *     planar [B,3,h,w] is (3hw, 1, hw), rows [B,N,3] are (3N, 3, 1); comp_stride = 1 rows are read with one 12-byte load.
 *   params fp32 [B,16] and model[b] as UdReconstruct.  T fp32 [nT,3,4] (nT = 1 or B; NULL = none): a rigid motion applied first, with
 *     UdSplat's arithmetic (x' = ((t00*x + t01*y) + t02*z) + t03, ...).
 *   Per model, every operation rounded separately, every maximum letting a NaN through:
 *     Pinhole     u = (fx*x + cx*z) / max(z, 0.01), v likewise (the skew-free K of the row)
 *     EUCM        d = sqrt(beta*(x*x + y*y) + z*z), den = max(alpha*d + (1 - alpha)*z, 1e-3), u = fx*(x/den) + cx
 *     Spherical   lon = atan2(x, z), lat = asin(y / max(|xyz|, 1e-5)), u = lon / (2 hfov2) * (Wp - 1) + (Wp - 1) / 2 with the ROW's Wp, Hp
 *     OPENCV      z -> 1e-9 sign(z) when |z| < 1e-9 (sign(0) = 0); ab = xy / z, r = |ab|; ab * (1 + k1 r^2 + k2 r^4 + k3 r^6); tangential
 *                 u += (2 xr^2 + rd) p0 + 2 xr yr p1 (v mirrored), thin prism u += s0 rd + s1 rd^2, v += s2 rd + s3 rd^2; then * f + c
 *     Fisheye624  the same front end; th = atan(r), th_k = th + sum_j k_j th^(3+2j) (j < 6) along ab / r (1, 1 where r < 1e-9); same tail
 *     MEI         ab = xy / (z + xi |xyz|); ab * (1 + k1 r^2 + k2 r^4); tangential (p at positions 6, 7); * f + c
 *   outputs: uv fp32, planar [B,2,n_points] (uv_rows = 0) or rows [B,n_points,2] (uv_rows != 0; one 8-byte store);
 *     inside uint8 [B,n_points] (optional): the model's own in-image test against the descriptor's H, W, comparisons as in the reference
 *       (Pinhole u >= 0 & u < W & v >= 0 & v < H; EUCM !(u < 0 | u > W | v < 0 | v > H | z' < 0); the others the same without z');
 *     depth fp32 [B,n_points] (optional): the model's depth of the point, z', or |xyz'| for Spherical -- what UdReconstruct multiplies with.
 *   Limits: 1 <= B <= UD_RECON_MAX_B, H, W >= 1, 0 <= n_points < 2^31, point_stride, comp_stride >= 1, batch_stride >= 0.  Every refusal
 *   is returned before any HIP call. */
typedef struct UdCameraProject {
  const float* xyz; const float* params; const float* T;
  float* uv; unsigned char* inside; float* depth;
  long long batch_stride, point_stride, comp_stride, n_points;
  int B, H, W, nT, uv_rows;
  unsigned char model[UD_RECON_MAX_B];
} UdCameraProject;
int ud_camera_project(const UdCameraProject* desc, void* stream);

/* And back: the viewing ray at ANY image coordinate, the device form of Camera.unproject / get_rays / reconstruct (utils/camera.py:
 * base :69-92, Pinhole :255-273, EUCM :307-328, Spherical :371-392, OPENCV :496-694, Fisheye624 :778-974, MEI :985-1082, BatchCamera
 * :1167-1171), one camera model per image, one thread per point (csrc/unproject.hip; the arithmetic is csrc/camera_models.h
 * ud_cam_unproject_*).  Stream-ordered, no host synchronisation.
 *   uv fp32: coordinate c of point r of image b is at uv[b * batch_stride + r * point_stride + c * comp_stride] (ELEMENTS), as
 *     UdCameraProject addresses xyz: planar [B,2,h,w] is (2hw, 1, hw), rows [B,N,2] are (2N, 2, 1); batch_stride = 0 is one coordinate
 *     set shared by every image.  uv = NULL: the identity grid of the descriptor's H, W at pixel centres u + 0.5, v + 0.5 (nothing is
 *     materialised; n_points must be H * W; the strides are not read).
 *   params fp32 [B,16] and model[b] as UdReconstruct.  depth fp32 [B,n_points] (optional).
 *   rays fp32, planar [B,3,n_points] (rays_rows = 0) or rows [B,n_points,3] (rays_rows != 0).  Every operation rounds separately, every
 *   maximum lets a NaN through (`x < m ? m : x`).  With depth = NULL and normalize = 0 the class's own unproject value, NOT normalised:
 *     Pinhole     r = ((u - cx) / fx, (v - cy) / fy, 1), no skew;  r / max(r.z, 1e-4).  r.z is NaN instead of 1 when an intrinsic or a
 *                 coordinate is not finite, so the whole ray is NaN then, as the reference's matrix product gives it
 *     EUCM        mx = (u - cx) / fx, my likewise, r2 = mx*mx + my*my, mz = (1 - beta alpha^2 r2) / (alpha sqrt(max(1 - (2 alpha - 1) beta r2,
 *                 1e-5)) + (1 - alpha)), c = 1 / sqrt(mx*mx + my*my + mz*mz + 1e-5);  (c mx, c my, max(c mz, 1e-3))
 *     Spherical   lon = (u - (Wp - 1) / 2) / (Wp - 1) * (2 hfov2) with the ROW's Wp, Hp, lat likewise; s = (cos lat sin lon, sin lat,
 *                 cos lat cos lon);  s / max(|s|, 1e-5)
 *     OPENCV, Fisheye624   (dx, dy, 1) of the solvers: 10 Newton iterations undoing tangential and thin-prism terms, the trust-region
 *                 loop on theta (at most 10 iterations), th / r (tan(th) / r for Fisheye624) along (xr, yr)
 *     MEI         (dx, dy, pz): 20 tangential and 20 radial Newton iterations, lifted with the mirror parameter xi; fully per point
 *   normalize != 0: that value / max(|value|, 1e-4), Camera.get_rays.  With depth the class's reconstruct rule, the expressions of
 *   ud_reconstruct (so the identity grid with a depth gives ud_reconstruct's bits):
 *     Pinhole r / max(r.z, 1e-4) * max(d, 0);  Spherical r * d;  the others r / max(r.z, 1e-4) * max(d, 1e-4), r as above
 *   normalize together with depth is refused.
 *   valid uint8 [B,n_points] (optional): the reference's unprojection_mask.  Pinhole: z of the stored ray > 1e-4.  EUCM: r2 < (alpha < 0.5
 *     ? 1e6 : 1 / (beta (2 alpha - 1))) and c mz > 1e-3, taken before the clamp.  Spherical, OPENCV, Fisheye624, MEI: 1 (no mask there).
 *   A batch without an OPENCV / Fisheye624 member is one launch.  Otherwise two after the clear: in the first every point of such an image runs its own
 *   10 trust-region steps in registers and each workgroup publishes the largest |residual| at theta_0 .. theta_10 (one atomicMax per
 *   workgroup and iteration); the second reads the iteration at which the image's maximum first fell below 1e-3, redoes that many steps and writes.
 *   Every image leaves the radial loop on the maximum over ITS OWN points, the points this call was given (the reference takes the maximum
 *   over the tensor its unproject receives); the iterates of a point depend on that point alone, so the result is that of an init / step /
 *   final launch sequence bit for bit, with no per-point state in memory.  The maxima are cleared by the call (a small launch of its own on
 *   `stream`), so a captured graph can be replayed with changed uv.
 *   work: device scratch, 16-byte aligned, of at least ud_camera_unproject_work_bytes(B, n_iterative) bytes (host-only query; -1 for
 *   arguments outside the limits): 11 maxima per iterative image.  May be NULL when there is no OPENCV / Fisheye624 member.
 *   Limits: 1 <= B <= UD_RECON_MAX_B, H, W >= 1, 0 <= n_points < 2^31 - 256, point_stride, comp_stride >= 1, batch_stride >= 0 (with uv).
 *   Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdCameraUnproject {
  const float* uv; const float* params; const float* depth;
  float* rays; unsigned char* valid;
  void* work; long long work_bytes;
  long long batch_stride, point_stride, comp_stride, n_points;
  int B, H, W, normalize, rays_rows;
  unsigned char model[UD_RECON_MAX_B];
} UdCameraUnproject;
int ud_camera_unproject(const UdCameraUnproject* desc, void* stream);
long long ud_camera_unproject_work_bytes(int B, int n_iterative);

/* Sampling with such coordinates: the maps of a batch at arbitrary image coordinates in ONE launch (csrc/remap.hip; the arithmetic of a
 * point is csrc/remap_taps.h).  A sampler and nothing else -- no camera arithmetic: the coordinates are ud_camera_project's uv of
 * ud_camera_unproject's rays (undistortion, backward warping), keypoints, or anything else.  No workspace, no atomics, no host
 * synchronisation: captures into a graph.
 *   src  [B or 1 (src_shared != 0), C, Hs, Ws] planar, contiguous, fp32 or uint8 (src_u8 != 0), any C >= 1.
 *   src_mask uint8 [B or 1 (mask_shared != 0), 1, Hs, Ws] (optional): a tap whose mask is 0 does not contribute.
 *   uv fp32, addressed as UdCameraUnproject's: coordinate c of point r of image b at uv[b * batch_stride + r * point_stride + c * comp_stride]
 *     (ELEMENTS); batch_stride = 0 shares one set.  Pixel centres at half-integers: the index-space position is x = u - 0.5, y = v - 0.5.
 *   coord_valid uint8 [B,n_points] (optional; ud_camera_project's `inside`): a point with 0 gets value 0 and valid 0.
 *   mode     UD_REMAP_NEAREST: the tap rint(x), rint(y), round half to even (grid_sample's nearbyint), the source's bits.
 *            UD_REMAP_BILINEAR: taps floor(x), floor(x) + 1 and the same in y; lx = x - floor(x), hx = 1 - lx;
 *              t0 = v00*hx + v01*lx, t1 = v10*hx + v11*lx, out = t0*hy + t1*ly, every operation rounded separately.
 *   padding  UD_REMAP_ZEROS: a tap outside the source contributes 0 (grid_sample padding_mode="zeros", align_corners=False).
 *            UD_REMAP_BORDER: x, y are clamped to [0, Ws - 1], [0, Hs - 1] first.
 *   normalize != 0 (bilinear): the same expression over the contributing taps (in range, src_mask != 0) divided by the same expression
 *     on 1 for those taps (their weight sum); 0 where that sum is 0.  The mode for depth maps with holes.
 *   out  fp32, planar [B,C,n_points] (out_rows = 0) or rows [B,n_points,C] (out_rows != 0); or uint8 (out_u8 != 0, uint8 sources only):
 *     rounded half to even and clamped to [0, 255].
 *   valid uint8 [B,n_points] (optional): 1 only if coord_valid is 1, both coordinates are finite, 0 <= u <= Ws and 0 <= v <= Hs, and at
 *     least one tap with a non-zero weight contributed.  A point whose coord_valid is 0 or whose coordinates are NaN or +-inf has out = 0
 *     in every channel; a finite coordinate outside the image is sampled as the padding says (that is what grid_sample returns there)
 *     with valid = 0.
 *   A coordinate never becomes an address before it is safe: NaN, +-inf and huge values are clamped in floating point (NaN to a fixed
 *   in-range value) before the conversion to an index.
 *   Limits: 1 <= B <= UD_RECON_MAX_B, C, Hs, Ws, n_points >= 1; n_points, C * n_points, C * Hs * Ws < 2^31 - 256; point_stride,
 *   comp_stride >= 1, batch_stride >= 0.  Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
enum { UD_REMAP_NEAREST = 0, UD_REMAP_BILINEAR = 1 };  /* UdRemap.mode */
enum { UD_REMAP_ZEROS = 0, UD_REMAP_BORDER = 1 };      /* UdRemap.padding */
typedef struct UdRemap {
  const void* src; const unsigned char* src_mask; const float* uv; const unsigned char* coord_valid;
  void* out; unsigned char* valid;
  long long batch_stride, point_stride, comp_stride, n_points;
  int B, C, Hs, Ws, mode, padding, normalize, src_u8, out_u8, out_rows, src_shared, mask_shared;
} UdRemap;
int ud_remap(const UdRemap* desc, void* stream);

/* The reference's Camera.mask_overlap_projection (utils/camera.py:132-154) for a batch in one launch: uv fp32 [B,2,H,W] (a projection of
 * the pixel grid's own points) -> mask uint8 [B,1,H,W].  One thread per pixel; the flow uv - (x + 0.5, y + 0.5) is formed at the pixel
 * and at each of the four taps, never stored.  Per pixel in fp32, every operation rounded separately: s = 0.1f * flow + id;
 * g = s / (W - 1) * 2 - 1; ix = ((g + 1) * W - 1) / 2 (grid_sample, align_corners=False); clamp to [0, W - 1] (NaN to 0); floor; corner
 * weights nw = (ix_se - ix) * (iy_se - iy), ...; sampled = nw v_nw + ne v_ne + sw v_sw + se v_se per component; norms sqrtf(a*a + b*b);
 * mask = (0.9f |flow| < |sampled|) | (|flow| < 1).  A NaN makes both comparisons false.
 * Limits: 1 <= B <= UD_RECON_MAX_B, H, W >= 2 (the reference divides by H - 1 and W - 1), H * W < 2^31 - 256. */
typedef struct UdOverlapMask {
  const float* uv; unsigned char* mask;
  int B, H, W;
} UdOverlapMask;
int ud_overlap_mask(const UdOverlapMask* desc, void* stream);

/* Backward warping: ud_camera_unproject -> ud_camera_project -> ud_remap fused into ONE launch with one thread per destination pixel
 * (csrc/warp.hip; the arithmetic of a pixel is csrc/warp_point.h, which only calls csrc/camera_models.h and csrc/remap_taps.h).  For every
 * pixel of a destination view: its point, a rigid motion, the projection through the source camera, the source view's maps sampled there,
 * the validity of the sample and an optional visibility test against the source's depth.  The point map, the coordinate map, the inside
 * mask and the projected depth stay in registers; every output has the bits the separate calls give.  No workspace, no atomics, no LDS,
 * no host synchronisation: captures into a graph.
 *   The point of destination pixel i = y * Wo + x of image b, exactly one of:
 *     points fp32 planar [B,3,Ho,Wo]: loaded (ud_reconstruct's or a network's point map).
 *     depth  fp32 [B,Ho,Wo] with params_dst fp32 [B,16] and model_dst[b]: ud_camera_unproject's identity grid with a depth, the pixel
 *            centre (x + 0.5, y + 0.5) through the model's reconstruct rule (Pinhole r / max(r.z, 1e-4) * max(d, 0); Spherical r * d;
 *            EUCM, MEI r / max(r.z, 1e-4) * max(d, 1e-4)).  Closed-form destination models only (Pinhole, EUCM, Spherical, MEI): an
 *            OPENCV / Fisheye624 member is REFUSED with UD_ERR_UNSUPPORTED -- its radial loop ends on a maximum over the whole image, so
 *            the caller runs ud_camera_unproject and passes points.  model_dst and params_dst are not read in the points form.
 *   T fp32 [nT,3,4] (nT = 1 or B; NULL = none): destination-camera to source-camera coordinates, ud_camera_project's arithmetic
 *     (x' = ((t00*x + t01*y) + t02*z) + t03, ...).
 *   params_src fp32 [B,16] and model_src[b] (all six models): (u, v) = ud_camera_project's coordinates of (x', y', z'), `inside` its
 *     in-image test against Hs, Ws, dproj its depth (z', or |xyz'| for Spherical).
 *   Coordinate validity cv = inside && dproj > 0, ANDed with valid_in[b,i] != 0 (uint8 [B,Ho,Wo], optional) and, in the depth form, with
 *     depth > 0 (false for a NaN).  The destination model's unprojection mask (ud_camera_unproject's `valid`) is deliberately NOT part of
 *     it, so both forms agree; pass it as valid_in where it is wanted.
 *   src [B or 1 (src_shared != 0), C, Hs, Ws], src_mask uint8 [B or 1 (mask_shared != 0), 1, Hs, Ws] (optional), mode, padding, normalize,
 *     src_u8, out_u8: UdRemap's, sampled at (u, v) with cv as its coord_valid.
 *   out  fp32 or uint8 (out_u8 != 0, uint8 sources only), planar [B,C,Ho,Wo]: UdRemap's out.  0 in every channel where cv is 0 or a
 *     coordinate is not finite.
 *   valid uint8 [B,Ho,Wo] (optional): UdRemap's valid -- cv, both coordinates finite, 0 <= u <= Ws, 0 <= v <= Hs, a tap of non-zero weight.
 *   visible uint8 [B,Ho,Wo] (optional; needs src_depth fp32 [B or 1 (depth_shared != 0), 1, Hs, Ws]): ds = src_depth sampled at the same
 *     taps with the same mode and padding, a tap contributing only if its src_depth > 0 and its src_mask != 0, bilinear in the normalised
 *     form; visible = (that sample is valid as above) && fabsf(ds - dproj) <= tol * dproj, every operation rounded separately, false for a
 *     NaN.  tol_bits holds the bit pattern of the fp32 relative tolerance tol (the descriptor has integer and pointer fields only).
 *   uv fp32 planar [B,2,Ho,Wo] (optional) and proj_depth fp32 [B,Ho,Wo] (optional): (u, v) and dproj of every pixel, valid or not.
 *   A coordinate never becomes an address before it is safe (csrc/remap_taps.h).
 *   Limits: 1 <= B <= UD_RECON_MAX_B, C, Ho, Wo, Hs, Ws >= 1; Ho * Wo, C * Ho * Wo, Hs * Ws, C * Hs * Ws < 2^31 - 256.  Every refusal is
 *   returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdWarpCamera {
  const void* src; const unsigned char* src_mask; const float* src_depth;
  const float* points; const float* depth; const float* params_dst; const float* params_src; const float* T;
  const unsigned char* valid_in;
  void* out; unsigned char* valid; unsigned char* visible; float* uv; float* proj_depth;
  int B, C, Ho, Wo, Hs, Ws, nT, mode, padding, normalize, src_u8, out_u8, src_shared, mask_shared, depth_shared, tol_bits;
  unsigned char model_dst[UD_RECON_MAX_B], model_src[UD_RECON_MAX_B];
} UdWarpCamera;
int ud_warp_camera(const UdWarpCamera* desc, void* stream);

/* Multi-view depth consistency and fusion in ONE launch (csrc/consistency.hip; the arithmetic of a pixel is csrc/consistency_point.h, which
 * only calls csrc/camera_models.h and csrc/remap_taps.h): the forward-backward geometric filter of multi-view stereo for every pixel of a
 * reference view against V neighbour views, one thread per reference pixel with the view loop inside it.  Per view it is ud_warp_camera ->
 * ud_camera_unproject -> ud_camera_project and the element-wise comparisons fused; every output has the bits the separate calls give.  No
 * workspace, no atomics, no LDS, no host synchronisation: captures into a graph.
 *   Reference pixel i = y * W + x of image b: depth fp32 [B,H,W], params_ref fp32 [B,16], model_ref[b].  ref_ok = depth > 0 (false for a
 *     NaN) && valid_in[b,i] != 0 (uint8 [B,H,W], optional).  P = ud_camera_unproject's identity grid with the depth at the pixel centre
 *     (x + 0.5, y + 0.5), computed once.
 *   View v = 0 .. V-1, in this order: src_depth fp32 [B,V,Hs,Ws], src_mask uint8 [B,V,Hs,Ws] (optional), params_src fp32 [V,B,16],
 *     model_src[v * B + b]; T and Tinv fp32 [nT,V,3,4] (nT = 1 or B sets of V matrices): reference-camera to view-camera coordinates and
 *     its inverse, ud_camera_project's arithmetic (x' = ((t00*x + t01*y) + t02*z) + t03, ...).
 *       Q = T P; (u, v) = the view's projection of Q, dproj its depth; cv = ref_ok && inside(u, v; Hs, Ws) && dproj > 0.
 *       ds = src_depth sampled at (u, v): bilinear, zeros padding, a tap contributing only if its depth > 0 and its src_mask != 0, the
 *         normalised form -- UdWarpCamera's out and valid for src = src_depth[b,v], src_mask = (src_depth > 0) & src_mask, normalize = 1.
 *       Q' = the view's reconstruct rule at (u, v) with ds; P' = Tinv Q'; (u', v') = the reference's projection of P', dback its depth.
 *       e2 = (u' - (x + .5))^2 + (v' - (y + .5))^2; diff = fabsf(dback - depth);
 *       consistent = valid sample && inside(u', v'; H, W) && dback > 0 && e2 <= px_tol * px_tol && diff <= rel_tol * depth, every
 *         operation rounded separately in fp32, false whenever anything is a NaN.  A consistent view adds dback to a running sum that
 *         starts at depth, in view order.
 *   fused fp32 [B,H,W]: sum / (float)(count + 1), 0 where ref_ok is false.  count uint8 [B,H,W]: the consistent views.  mask uint8
 *     [B,H,W]: ref_ok && count >= min_views.  Optional per-view maps [B,V,H,W]: consistent uint8, err_px fp32 (sqrtf(e2)), err_rel fp32
 *     (diff / depth); the error maps are 0 where the sample is not valid.
 *   px_tol_bits / rel_tol_bits hold the bit patterns of the fp32 tolerances (the descriptor has integer and pointer fields only).
 *   Closed-form models only (Pinhole, EUCM, Spherical, MEI): an OPENCV / Fisheye624 member, reference or view, is REFUSED with
 *   UD_ERR_UNSUPPORTED -- its unprojection ends on a maximum over the whole image.  A coordinate never becomes an address before it is
 *   safe (csrc/remap_taps.h).
 *   Limits: B, V >= 1, B * V <= UD_RECON_MAX_B, V <= 255, H, W, Hs, Ws >= 1; H * W, Hs * Ws, V * Hs * Ws < 2^31 - 256; nT 1 or B; px_tol,
 *   rel_tol finite and >= 0; 0 <= min_views <= V.  Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdDepthConsistency {
  const float* depth; const float* params_ref; const unsigned char* valid_in;
  const float* src_depth; const unsigned char* src_mask; const float* params_src; const float* T; const float* Tinv;
  float* fused; unsigned char* count; unsigned char* mask; unsigned char* consistent; float* err_px; float* err_rel;
  int B, V, H, W, Hs, Ws, nT, min_views, px_tol_bits, rel_tol_bits;
  unsigned char model_ref[UD_RECON_MAX_B], model_src[UD_RECON_MAX_B];
} UdDepthConsistency;
int ud_depth_consistency(const UdDepthConsistency* desc, void* stream);

/* Depth views fused into a truncated signed distance (TSDF) volume in ONE launch (csrc/tsdf.hip; the arithmetic of a voxel is
 * csrc/tsdf_point.h, which only calls csrc/camera_models.h and csrc/remap_taps.h): every voxel centre is projected into every view, the
 * view's depth is read at the nearest pixel and the truncated distance is averaged into the voxel, one thread per voxel with the view loop
 * inside it.  Per view it is ud_camera_project -> ud_remap (nearest) and the element-wise update fused; every output has the bits the
 * separate calls give.  No workspace, no atomics, no LDS, no host synchronisation: captures into a graph.
 *   Volume b: tsdf, weight fp32 [B,Nz,Ny,Nx] (x fastest), color fp32 planar [B,3,Nz,Ny,Nx] (with image, else NULL), count uint8
 *     [B,Nz,Ny,Nx] (optional: the views that updated the voxel in this call).  Voxel i = (iz * Ny + iy) * Nx + ix has the centre
 *     p = origin + ((float)index + 0.5f) * voxel_size per axis, origin fp32 [n_origin,3], n_origin = 1 (shared) or B.
 *     fresh != 0: the state starts at tsdf = 1, weight = 0, color = 0 and the volume's memory is not read; otherwise it is read.
 *   View v = 0 .. V-1, in this order: src_depth fp32 [B,V,Hs,Ws], src_mask uint8 [B,V,Hs,Ws] (optional), src_weight fp32 [B,V,Hs,Ws]
 *     (optional), image uint8 [B,V,3,Hs,Ws] (optional), params fp32 [V,B,16], model[v * B + b]; T fp32 [nT,V,3,4] (nT = 1 or B sets of V
 *     matrices): volume (world) to view-camera coordinates, ud_camera_project's arithmetic.
 *       q = T p; (u, w) = the view's projection of q, d its depth, inside its in-image test against (Hs, Ws).
 *       One nearest tap at (u, w), zeros padding (csrc/remap_taps.h); it contributes when src_depth there is > 0 and src_mask != 0.
 *       valid = inside && u, w finite && 0 <= u <= Ws && 0 <= w <= Hs && the tap contributes (UdRemap's valid for coord_valid = inside and
 *         src_mask = (src_depth > 0) & src_mask).  ds = the depth at the tap, wv = src_weight there (1 without), rgb = image's bytes there.
 *       sdf = ds - d; obs = valid && d > 0 && sdf >= -trunc && wv > 0 && wv <= FLT_MAX (false whenever a NaN is involved);
 *       s = fminf(sdf / trunc, 1).  If obs: Wn = weight + wv; tsdf = (tsdf * weight + s * wv) / Wn; color[k] = (color[k] * weight + rgb[k]
 *         * wv) / Wn; weight = has_max_weight ? fminf(Wn, max_weight) : Wn; ++count.  Every operation rounded separately in fp32.
 *   voxel_size_bits / trunc_bits / max_weight_bits hold the bit patterns of the fp32 values (the descriptor has integer and pointer fields
 *   only).  All six camera models (projection is closed form for each).  A coordinate never becomes an address before it is safe.
 *   Limits: B, V >= 1, B * V <= UD_RECON_MAX_B, V <= 255, Nx, Ny, Nz, Hs, Ws >= 1; Nx * Ny * Nz, Hs * Ws, V * 3 * Hs * Ws < 2^31 - 256; nT
 *   and n_origin 1 or B; voxel_size, trunc finite and > 0; max_weight finite and > 0 when has_max_weight != 0; image and color both or
 *   neither.  Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdTsdfIntegrate {
  const float* src_depth; const unsigned char* src_mask; const float* src_weight; const unsigned char* image;
  const float* params; const float* T; const float* origin;
  float* tsdf; float* weight; float* color; unsigned char* count;
  int B, V, Nx, Ny, Nz, Hs, Ws, nT, n_origin, fresh, has_max_weight, voxel_size_bits, trunc_bits, max_weight_bits;
  unsigned char model[UD_RECON_MAX_B];
} UdTsdfIntegrate;
int ud_tsdf_integrate(const UdTsdfIntegrate* desc, void* stream);

/* The surface of a TSDF volume as packed points (csrc/tsdf.hip): UdPointCloud's ordered, deterministic compaction (flag + count, scan,
 * pack; no atomics, no host synchronisation) over SLOTS instead of pixels.  Slot s = 3 * voxel + axis of volume b is the edge from the
 * voxel to its +x (axis 0) / +y (1) / +z (2) neighbour.  It is live when the neighbour lies in the grid, both weights are >= min_weight,
 * a = tsdf[voxel] and b = tsdf[neighbour] are both not NaN and (a < 0) != (b < 0).  Its row: t = a / (a - b); xyz = the voxel's centre
 * (UdTsdfIntegrate's) with coordinate [axis] moved by t * voxel_size; colour c0[k] + t * (c1[k] - c0[k]), stored as fp32 (rgb_f32 != 0) or
 * rounded half to even and clamped to a byte.  Every operation rounded separately in fp32.
 *   inputs: tsdf, weight fp32 [B,Nz,Ny,Nx]; color fp32 [B,3,Nz,Ny,Nx] or NULL; origin fp32 [n_origin,3], n_origin = 1 or B.
 *   Order: volumes in batch order, slots ascending inside a volume.  Bitwise reproducible.
 *   outputs: counts int64 [B] and offsets int64 [B+1] are always written, with the TRUE totals whatever `capacity` is.  xyz == NULL: count
 *     only.  Otherwise, for the rows r < min(total, capacity): xyz fp32 [capacity,3]; rgb [capacity,3] u8 or fp32 (optional, needs color).
 *     Rows r >= capacity are dropped, rows r >= total never written.
 *   work: device scratch of at least ud_tsdf_points_work_bytes(B, Nx, Ny, Nz) bytes (host-only query; -1 outside the limits), 8-byte
 *     aligned, work_bytes its size.  Its contents need no initialisation.
 *   Limits: 1 <= B <= 65535, Nx, Ny, Nz >= 1, 3 * Nx * Ny * Nz < 2^31 - 256, capacity >= 0, voxel_size finite and > 0, min_weight not a
 *   NaN.  Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdTsdfPoints {
  const float* tsdf; const float* weight; const float* color; const float* origin;
  float* xyz; void* rgb; long long* counts; long long* offsets;
  void* work; long long work_bytes;
  long long capacity;
  int B, Nx, Ny, Nz, n_origin, rgb_f32, voxel_size_bits, min_weight_bits;
} UdTsdfPoints;
int ud_tsdf_points(const UdTsdfPoints* desc, void* stream);
long long ud_tsdf_points_work_bytes(int B, int Nx, int Ny, int Nz);

/* The surface of a TSDF volume as an indexed triangle mesh (csrc/tsdf_mesh.hip; the arithmetic of a cell and of a quad is
 * csrc/tsdf_mesh_point.h): naive surface nets as two of UdTsdfPoints' ordered compactions, one over cells and one over slots; no case
 * table, no atomics, no host synchronisation.  The volume, min_weight, the voxel centres, the slots and a slot's crossing point and
 * colour are UdTsdfPoints'.  Every operation rounded separately in fp32.
 *   Cells.  The cell of voxel i = (iz * Ny + iy) * Nx + ix has the corners (ix + dx, iy + dy, iz + dz), d* in {0, 1}; it exists when
 *     ix + 1 < Nx, iy + 1 < Ny and iz + 1 < Nz.  It is live when all eight weights are >= min_weight, no corner distance is a NaN and the
 *     corners are not all of one sign (d < 0 is the sign).  A grid with an axis of one voxel has no cells: an empty mesh.
 *   Vertices: one per live cell; volumes in batch order, then cells in voxel order.  The cell's edges e = 4 * axis + k, k = 0..3: with
 *     (o0, o1) the two other axes ascending, the edge's lower voxel is the cell's voxel moved by k & 1 along o0 and (k >> 1) & 1 along o1,
 *     and the edge is slot 3 * lower + axis.  The vertex is the sum of the live slots' crossing points in edge order (the first one
 *     initialises the sum) divided by (float)their number; rgb the same mean of the slots' colours, stored as fp32 (rgb_f32 != 0) or
 *     rounded half to even and clamped to a byte.  normals: g[axis] = the sum in edge order of (d1 - d0) over the axis' four edges,
 *     len = sqrtf((g0 * g0 + g1 * g1) + g2 * g2), g / len, or (0, 0, 0) when len is not finite and positive; it points to the positive side.
 *   Faces: a live slot with (u, v) = ((axis + 1) % 3, (axis + 2) % 3) and voxel c yields one quad when the cells q0 = c - e_u - e_v,
 *     q1 = c - e_v, q2 = c, q3 = c - e_u exist and are live.  Winding (q0, q1, q2, q3) when tsdf[c] < 0, else (q0, q3, q2, q1): the
 *     geometric normal points to the positive side.  The quad (a, b, c, d) becomes the triangles (a, b, c) and (a, c, d), rows 2r and
 *     2r + 1 of quad r; volumes in batch order, then slots ascending.  The indices are int32 vertex rows LOCAL to the volume (the row
 *     minus vert_offsets[b]).  A live cell none of whose quads is complete leaves an unreferenced vertex.
 *   outputs: vert_counts / face_counts int64 [B] and vert_offsets / face_offsets int64 [B+1] are always written, with the TRUE totals
 *     (faces in triangles) whatever the capacities are.  vertices fp32 [vert_capacity,3], rgb [vert_capacity,3] u8 or fp32 (optional,
 *     needs color and vertices), normals fp32 [vert_capacity,3] (optional, needs vertices): the rows r < min(total, vert_capacity).  faces
 *     int32 [face_capacity,3]: a quad is written only when both its triangles lie below face_capacity.  vertices == NULL or
 *     vert_capacity == 0, faces == NULL or face_capacity == 0: that part is counted only.  Absent outputs are never touched.
 *   work: device scratch of at least ud_tsdf_mesh_work_bytes(B, Nx, Ny, Nz) bytes (host-only query; -1 outside the limits), 8-byte
 *     aligned, work_bytes its size.  Its contents need no initialisation.
 *   Limits: UdTsdfPoints'.  Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdTsdfMesh {
  const float* tsdf; const float* weight; const float* color; const float* origin;
  float* vertices; void* rgb; float* normals; int* faces;
  long long* vert_counts; long long* vert_offsets; long long* face_counts; long long* face_offsets;
  void* work; long long work_bytes;
  long long vert_capacity, face_capacity;
  int B, Nx, Ny, Nz, n_origin, rgb_f32, voxel_size_bits, min_weight_bits;
} UdTsdfMesh;
int ud_tsdf_mesh(const UdTsdfMesh* desc, void* stream);
long long ud_tsdf_mesh_work_bytes(int B, int Nx, int Ny, int Nz);

/* Frame-to-model point-to-plane ICP, one Gauss-Newton step in TWO launches (csrc/icp.hip; the arithmetic is csrc/icp_point.h, which only
 * calls csrc/camera_models.h and csrc/remap_taps.h): a depth frame, or a point map, aligned to the point and normal maps of a model view
 * (what ud_tsdf_render returns) under the current estimate T, frame camera to model camera.  KinectFusion's tracking step.
 *   Frame pixel i = y * W + x of image b: depth fp32 [B,H,W] with params fp32 [B,16] and model_frame[b] (closed-form models only: Pinhole,
 *     EUCM, Spherical, MEI), or points fp32 [B,3,H,W] in its place (exactly one of the two; the route of OPENCV / Fisheye624 frames).
 *     p = ud_reconstruct's point of the pixel centre (x + 0.5, y + 0.5), or the point as given.  live = depth > 0 (points: every component
 *     finite) && mask[b,i] != 0 (uint8, optional) && weights[b,i] > 0 and finite (fp32, optional; w = 1 without).
 *   q = T p, ud_camera_project's arithmetic; (u, v) = the projection of q through params_model fp32 [B,16], model_model[b] (any of the six);
 *     usable = the model's in-image test against (Hm, Wm) && the model's depth of q > 0 && u, v finite.
 *   The model at the nearest pixel (ud_remap's nearest tap, zeros padding): m = model_points, n = model_normals fp32 [B,3,Hm,Wm], read only
 *     where the tap is in range and model_valid uint8 [B,Hm,Wm] != 0 (0 otherwise); the model pixel is valid then if also 0 <= u <= Wm and
 *     0 <= v <= Hm.
 *   e = m - q; d2 = (e0*e0 + e1*e1) + e2*e2; r = (n0*e0 + n1*e1) + n2*e2; c = q x n (c0 = q1*n2 - q2*n1, cyclic); every operation rounded
 *     separately in fp32.  matched = live && usable && model pixel valid && n != 0 && d2 <= dist_tol * dist_tol && (with normals fp32
 *     [B,3,H,W] and has_cos: (R_T nf) . n >= cos_tol, products summed left to right) && r, c, n finite; false whenever a NaN is compared.
 *   The row g = (c0, c1, c2, n0, n1, n2).  Optional per-pixel outputs matched uint8 [B,H,W], residual fp32 [B,H,W], rows fp32 [B,6,H,W]:
 *     exactly 0 where not matched.
 *   system fp64 [B,32], over the matched pixels: gw_i = (double)w * (double)g_i; A_ij += gw_i * (double)g_j for i <= j (slots 0..20, the
 *     upper triangle row-major), b_i += gw_i * (double)r (21..26), e += ((double)w * (double)r) * (double)r (27), wsum (28), count (29,
 *     exact), 30 and 31 zero.  Summed in a fixed order -- a thread's pixels in order, the wave's threads by the xor butterfly, the waves in
 *     order, the workgroups in index order: no floating-point atomics, the bits do not depend on scheduling or on the workspace's contents.
 *   work: device scratch of at least ud_icp_workspace_bytes(B, H, W) bytes (host-only query; -1 outside the limits), 8-byte aligned, holding
 *     the workgroups' partials [B, nblk, 32], nblk = min(ceil(H * W / 256), 256) workgroups per image.  blocks != 0 replaces the 256 (at
 *     most 1024, which is what the workspace is sized for): another order of summation, for measurement.
 *   solve != 0: the second launch also solves (A + damping I) x = b by LDL^T without pivoting in fp64 (+ - * / only) and, when count >=
 *     min_count, every pivot > 0 and x finite (status 1), sets T[b] = [R R_old | R t_old + v] in place with R the Cayley map of omega / 2,
 *     formed in fp64 and rounded to fp32 once; status 0 leaves T[b] as it was and x = 0.  It needs nT = B.  x fp64 [B,6], status uint8 [B]
 *     and stats fp64 (4 values e, wsum, count, status at stats + b * stats_stride) are optional.  The order of every operation is fixed in
 *     the comments of csrc/icp_point.h.  damping_bits holds the bit pattern of the fp64 damping, dist_tol_bits / cos_tol_bits those of the
 *     fp32 tolerances.
 *   ud_icp_update: the second launch alone, on a given system (T, system, nT = B, damping, min_count, x, status, stats are read).
 *   Limits: 1 <= B <= UD_RECON_MAX_B; H, W, Hm, Wm >= 1; 6 * H * W and 3 * Hm * Wm < 2^31 - 256; nT 1 or B; dist_tol and damping finite and
 *   >= 0; -1 <= cos_tol <= 1; min_count >= 0; 0 <= blocks <= 1024.  Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdIcp {
  const float* depth; const float* points; const float* params; const unsigned char* mask; const float* weights; const float* normals;
  const float* model_points; const float* model_normals; const unsigned char* model_valid; const float* params_model;
  float* T; void* work; double* system; unsigned char* matched; float* residual; float* rows; double* x; unsigned char* status; double* stats;
  long long work_bytes, stats_stride, damping_bits;
  int B, H, W, Hm, Wm, nT, solve, min_count, has_cos, dist_tol_bits, cos_tol_bits, blocks;
  unsigned char model_frame[UD_RECON_MAX_B], model_model[UD_RECON_MAX_B];
} UdIcp;
int ud_icp_linearize(const UdIcp* desc, void* stream);
int ud_icp_update(const UdIcp* desc, void* stream);
long long ud_icp_workspace_bytes(int B, int H, int W);

/* The depth pyramid of a batch in ONE launch (csrc/pyramid.hip; the arithmetic of a pixel is csrc/pyramid_point.h, where the definition is
 * written out operation by operation): an edge-preserving bilateral filter at level 0 and gated 2 x 2 means for levels 1 .. levels - 1,
 * what a coarse-to-fine tracker runs between the depth prediction and ud_icp_linearize.
 *   depth fp32 [B,H,W]; mask uint8 [B,H,W] (optional); weights fp32 [B,H,W] (optional).  A pixel is live when mask != 0 and
 *   0 < depth < +inf and, with weights, 0 < w < +inf (false for a NaN).  A pixel that is not live is 0 at every level.
 *   Level 0, radius r = 0: the live depths.  r >= 1: over the live taps inside the image, dy = -r..r (outer), dx = -r..r (inner):
 *   delta = |d - dc|, bin = delta * inv_bin >= 256 ? 255 : (int)(delta * inv_bin), w = ws[(dy+r)(2r+1) + dx+r] * wr[bin], num += w * d,
 *   den += w, out = num / den.  ws fp32 [(2r+1)^2] and wr fp32 [256] are DEVICE pointers; the caller keeps ws[centre] > 0 and wr[0] > 0
 *   (den > 0 follows); inv_bin_bits is the bit pattern of the fp32 inv_bin.  The level-0 weight is the centre's where live, else 0.
 *   Level l >= 1: H_l = H_{l-1} / 2, W_l = W_{l-1} / 2 (an odd last row or column is dropped); the members (2y,2x), (2y,2x+1),
 *   (2y+1,2x), (2y+1,2x+1) of level l - 1 are live where > 0; anchor = the smallest live member; a member is included when live and
 *   d - anchor <= gate (gate_bits: the fp32's bit pattern, >= 0, +inf allowed); value = the included members summed in that order / their
 *   count, weight = their weights summed likewise / the same count; 0 when no member is live.
 *   out_depth[l] fp32 [B,H_l,W_l], out_weights[l] likewise (read only with weights): a NULL pointer means that level is not written.
 *   tile: the level-0 tile of a workgroup, 0 = the default, 1 = 32 x 32, 2 = 64 x 16; the result does not depend on it.
 *   No workspace, no atomics, no host synchronisation: captures into a graph.
 *   Limits: 1 <= B <= UD_RECON_MAX_B, 1 <= levels <= 4, H, W >= 2^(levels-1), H * W < 2^31 - 256, 0 <= radius <= 4, gate >= 0 and not a
 *   NaN, inv_bin finite and > 0 (with a radius).  Every refusal is returned before any HIP call.  Built with -ffp-contract=off. */
typedef struct UdDepthPyramid {
  const float* depth; const unsigned char* mask; const float* weights; const float* ws; const float* wr;
  float* out_depth[4]; float* out_weights[4];
  int B, H, W, levels, radius, tile, gate_bits, inv_bin_bits;
} UdDepthPyramid;
int ud_depth_pyramid(const UdDepthPyramid* desc, void* stream);

/* A TSDF volume ray-cast to depth, points, normals and colour in ONE launch (csrc/tsdf_render.hip; the arithmetic of a ray is
 * csrc/tsdf_ray.h, where the definition is written out operation by operation): one thread per output pixel marches K samples through
 * the volume, reads the distance trilinearly and stops at the first crossing seen from the front.  No workspace, no atomics, no LDS, no
 * host synchronisation: captures into a graph.
 *   Volume b: tsdf, weight fp32 [B,Nz,Ny,Nx] (x fastest), color fp32 planar [B,3,Nz,Ny,Nx] or NULL, origin fp32 [n_origin,3] (n_origin 1
 *     or B) and voxel_size as UdTsdfIntegrate's.  T fp32 [nT,3,4] (nT = 1 or B) or NULL (identity): CAMERA TO VOLUME coordinates.
 *   Pixel (py, px) of image b, Ho x Wo: the direction d is the three values of rays (fp32 planar [B,3,Ho,Wo]) as they are, or, with rays
 *     NULL, ud_camera_unproject's normalised ray of (px + 0.5, py + 0.5) through model[b] / params fp32 [B,16] (closed-form models only:
 *     Pinhole, EUCM, Spherical, MEI).  With rays the model only selects the depth: the distance for Spherical, z otherwise.
 *   Sample k = 0 .. K-1: t = near + (float)k * step; p = T (t d); g_a = (p_a - origin_a) / voxel_size - 0.5 per axis.  In the grid when
 *     0 <= g_a <= N_a - 1 on every axis; then i_a = max(min((int)floorf(g_a), N_a - 2), 0), the upper corner min(i_a + 1, N_a - 1),
 *     f_a = g_a - i_a.  Valid when in the grid, all eight corner weights >= min_weight and the value s is not a NaN; s is the trilinear
 *     interpolant a + f * (b - a) along x, then y, then z.
 *   Scan in order, the previous and the current sample both valid: !(s_prev < 0) && s < 0 is the hit; s_prev < 0 && !(s < 0) ends the
 *     ray without one (the surface seen from behind).  An invalid sample resets the previous one.
 *   At the hit: al = s_prev / (s_prev - s); t* = t_(k-1) + al * (t_k - t_(k-1)); points = q* = t* d (camera frame); depth =
 *     the model's depth of q*; valid = hit && depth > 0, every output of a pixel that is not valid is exactly 0.  normals: the analytic
 *     gradient of the interpolant at both samples blended with al, rotated by T's rotation transposed, divided by its largest magnitude
 *     and by its length, turned towards the viewer (n . q* <= 0), exactly 0 where not finite or zero.  color_out: the trilinear colours
 *     of both samples blended with al, planar [B,3,Ho,Wo], fp32 (color_f32 != 0) or rounded half to even and clamped to a byte.
 *   Outputs: depth fp32 [B,Ho,Wo] and valid uint8 [B,Ho,Wo] always; points, normals fp32 planar [B,3,Ho,Wo] and color_out optional.
 *   full_scan != 0: every sample is visited; otherwise the samples that cannot lie in the grid (a conservative ray / box intersection)
 *     are skipped, which changes no output bit.  wave_patch != 0: a wave renders an 8 x 8 pixel patch instead of 64 pixels of a row; no
 *     output bit depends on it.  voxel_size_bits / near_bits / step_bits / min_weight_bits hold the bit patterns of the fp32 values.
 *   Limits: 1 <= B <= UD_RECON_MAX_B; Ho, Wo, Nx, Ny, Nz >= 1; Nx * Ny * Nz and 3 * Ho * Wo < 2^31 - 256; nT (with T) and n_origin 1 or
 *   B; voxel_size and step finite and > 0; near finite and >= 0; min_weight not a NaN; 1 <= K <= 16384; model tags 1..6, OPENCV and
 *   Fisheye624 only with rays; params with rays NULL; color_out only with color.  Every refusal is returned before any HIP call.  Built
 *   with -ffp-contract=off. */
typedef struct UdTsdfRender {
  const float* tsdf; const float* weight; const float* color; const float* origin; const float* T; const float* params; const float* rays;
  float* depth; unsigned char* valid; float* points; float* normals; void* color_out;
  int B, Ho, Wo, Nx, Ny, Nz, nT, n_origin, K, color_f32, full_scan, wave_patch, voxel_size_bits, near_bits, step_bits, min_weight_bits;
  unsigned char model[UD_RECON_MAX_B];
} UdTsdfRender;
int ud_tsdf_render(const UdTsdfRender* desc, void* stream);

/* Surface normals of a point map, or of a depth map seen through a camera, in ONE launch (csrc/normals.hip; the arithmetic of a pixel is
 * csrc/normals_point.h, where the definition is written out operation by operation).  Exactly one of:
 *     points fp32 planar [B,3,H,W]: the points form.  depth fp32 [B,H,W] is optional there and only feeds the edge test (P.z otherwise).
 *     depth  fp32 [B,H,W] with params fp32 [B,16] and model[b] (points NULL): the depth form.  The point of a pixel is ud_reconstruct's at
 *            the pixel centre, computed once per tile with a one-pixel halo and kept in LDS; ok additionally needs depth > 0.  Closed-form
 *            models only (Pinhole, EUCM, Spherical, MEI): an OPENCV / Fisheye624 member is REFUSED with UD_ERR_UNSUPPORTED -- its radial
 *            loop ends on a maximum over the whole image, so the caller runs ud_camera_unproject and passes points.
 *   mask uint8 [B or 1 (mask_shared != 0), H, W] (optional): pixels with 0 are not ok.
 *   A neighbour (left, right, up, down) is usable when it is inside the image, ok, and, with has_rtol != 0, |d[c] - d[q]| <= rtol *
 *   min(d[c], d[q]) (rtol_bits holds the bit pattern of the fp32 rtol; false for a NaN).  dx = P[R] - P[L], or one-sided with P[c] when
 *   only one of the two is usable; dy likewise with down and up; n = cross(dy, dx) / its largest magnitude, then / its length, negated
 *   when n . P[c] > 0, so every valid normal faces the viewer.  A pixel is valid when it is ok, both differences exist and the largest
 *   magnitude is > 0 and finite.
 *   normals fp32 planar [B,3,H,W]: exactly 0 where not valid.  valid uint8 [B,H,W] (optional).  rgb uint8 planar [B,3,H,W] (optional):
 *   floor((n + 1) * 127.5 + 0.5) clamped to 0..255, 0 where not valid.  No alignment is required of any pointer beyond its element's.
 *   No workspace, no atomics, no host synchronisation: captures into a graph.
 *   Limits: 1 <= B <= UD_RECON_MAX_B, H, W >= 1, H * W < 2^31 - 256, rtol finite and >= 0.  Every refusal is returned before any HIP
 *   call.  Built with -ffp-contract=off. */
typedef struct UdNormals {
  const float* points; const float* depth; const float* params; const unsigned char* mask;
  float* normals; unsigned char* valid; unsigned char* rgb;
  int B, H, W, mask_shared, has_rtol, rtol_bits;
  unsigned char model[UD_RECON_MAX_B];
} UdNormals;
int ud_normals(const UdNormals* desc, void* stream);

/* Normal-error metrics of a batch, per image, without a host synchronisation (csrc/normals.hip).  Per pixel with mask != 0 and all six
 * values finite: lg = sqrt((gx*gx + gy*gy) + gz*gz), lp likewise; dropped unless both are > 0 and finite; c = ((gx*px + gy*py) + gz*pz)
 * / (lg * lp) clamped to [-1, 1] (a NaN quotient is dropped); the error is acosf(c).
 *   gt, pred fp32 planar [B,3,H,W]; mask uint8 [B or 1 (mask_shared != 0), H, W] (optional).
 *   out fp32 [3 + T, B]: mean, median, rmse in degrees, then for each threshold the share of pixels with c > cos_t, i.e. an error strictly
 *     below it, as (float)count / (float)n.  cos_bits[t] holds the bit pattern of the fp32 rounding of the float64 cosine, computed by
 *     the host.  NaN rows for an image without a usable pixel.
 *   count int64 [B]: the usable pixels of each image.
 *   error fp32 [B,H,W] (optional): (float)((double)acosf(c) * 180 / pi), NaN where dropped.
 *   Sums are fp64 in a fixed order (thread, wave, block, chunk); only integer counts meet an atomic: two calls give the same bits.  The
 *   median is the exact lower median of the error (torch.median): a radix select on the order-preserving keys of c for the rank
 *   floor((n - 1) / 2) counted from the largest c, and one acosf.  workspace: at least ud_eval_normals_work_bytes(B, H, W, T) bytes
 *   (host-only query; -1 outside the limits), 16-byte aligned; its contents on entry do not matter.
 *   Limits: 1 <= B <= UD_RECON_MAX_B, H, W >= 1, H * W < 2^31 - 4096, 1 <= T <= UD_EVAL_NORMALS_MAX_T.  Every refusal is returned before
 *   any HIP call.  Built with -ffp-contract=off. */
#define UD_EVAL_NORMALS_MAX_T 8
typedef struct UdEvalNormals {
  const float* gt; const float* pred; const unsigned char* mask;
  float* out; long long* count; float* error;
  int B, H, W, T, mask_shared;
  int cos_bits[UD_EVAL_NORMALS_MAX_T];
} UdEvalNormals;
int ud_eval_normals(const UdEvalNormals* desc, void* workspace, long long bytes, void* stream);
long long ud_eval_normals_work_bytes(int B, int H, int W, int T);

/* ---- output side: the valid pixels of a batch of predictions as packed point-cloud rows (csrc/pointcloud.hip) ----
 * The device form of the reference's get_pointcloud_from_rgbd (unidepth/utils/visualization.py:57-104: numpy, one image per call) for a
 * whole batch: an ordered, deterministic stream compaction in a few plain launches on `stream` (flag + count, scan, pack), no atomics,
 * no float reduction, no workgroup waiting on another, no host synchronisation.
 *   inputs, all device, contiguous:  points fp32 [B,3,H,W] and / or depth fp32 [B,H,W] (at least one); K fp32 [nK,3,3], nK = 1 (shared)
 *     or B, needed when points is NULL; image u8 [B,3,H,W] or image_f32 fp32 [B,3,H,W] (at most one; both NULL = no colour);
 *     mask u8 [B,H,W] or NULL; confidence fp32 [B,H,W] or NULL.
 *   Predicate, all compares in fp32; d = depth[b,y,x] when depth is given, else points[b,2,y,x].  A pixel is kept when all hold:
 *     mask == NULL || mask[b,y,x] != 0
 *     points[b,0..2,y,x] all finite when points is given, else d finite
 *     UD_PC_MINCONF:  confidence[b,y,x] >= min_conf                       (NaN fails)
 *     UD_PC_RANGE:    d >= dmin && d <= dmax
 *     UD_PC_EDGE:     fabsf(d - dn) <= edge_rtol * fminf(d, dn) for every in-image 4-neighbour dn of the same depth source (neighbours
 *                     outside the image are skipped; a NaN or inf neighbour makes the compare false, so the pixel is dropped; the
 *                     neighbour's own mask is not consulted)
 *   Coordinates:  points given: points[b,:,y,x] copied bit-exactly.  Otherwise (depth mode), with fx, fy, cx, cy = K[.][0][0], [1][1],
 *     [0][2], [1][2] of K[b] (K[0] when nK = 1; skew is ignored, as in the reference) and every operation rounded to fp32 separately:
 *     x = ((float)u - cx) * d / fx,  y = ((float)v - cy) * d / fy,  z = d.  UD_PC_FLIP_Y negates y in either mode (the reference's +y up).
 *   Order: images in batch order, pixels row-major inside an image (numpy boolean indexing).  Bitwise reproducible.
 *   outputs:  counts int64 [B] = kept pixels per image and offsets int64 [B+1] = their exclusive prefix (offsets[B] = the total) are always
 *     written, with the TRUE totals whatever `capacity` is.  xyz == NULL: count only, nothing else is written.  Otherwise, for the rows
 *     r < min(total, capacity): xyz fp32 [capacity,3]; rgb [capacity,3] u8 (image) or fp32 (image_f32), not written without a colour
 *     input; index int32 [capacity] = y*W+x inside the image, or NULL.  Rows r >= capacity are dropped, rows r >= total never written.
 *   work: device scratch of at least ud_pointcloud_work_bytes(B, H, W) bytes (host-only query; one bit per pixel rounded up to tiles of
 *     1024, plus two int32 per tile), 8-byte aligned, work_bytes its size.  Its contents need no initialisation.
 *   Limits: 1 <= B <= 65535, H, W >= 1, H*W < 2^31 (B*H*W < 2^31 when index is given), capacity >= 0. */
enum { UD_PC_MINCONF = 1, UD_PC_RANGE = 2, UD_PC_EDGE = 4, UD_PC_FLIP_Y = 8 };
typedef struct UdPointCloud {
  const float* points; const float* depth; const float* K;
  const unsigned char* image; const float* image_f32; const unsigned char* mask; const float* confidence;
  float* xyz; void* rgb; int* index; long long* counts; long long* offsets;
  void* work; long long work_bytes;
  long long capacity;
  int B, H, W, nK, flags;
  float min_conf, dmin, dmax, edge_rtol;
} UdPointCloud;
int ud_pointcloud_pack(const UdPointCloud* desc, void* stream);
long long ud_pointcloud_work_bytes(int B, int H, int W);

/* ---- validation side: network-resolution maps brought to the ground truth's size (csrc/matchgt.hip) ----
 * The device form of the reference's match_gt / match_intrinsics (unidepth/utils/misc.py:596-690: per image, slice the padded window,
 * F.interpolate(bilinear, align_corners=False) to the target window, F.pad with zeros, torch.cat -- once per map) for a whole batch
 * whose images carry DIFFERENT paddings: ONE launch on `stream`, no atomics, no workspace, no host synchronisation, bitwise reproducible.
 *   Geometry, shared by every plane: source maps are h1 x w1, destinations H2 x W2.  pads1 / pads2: device int32 [B,4] in (left, right,
 *     top, bottom) order, or NULL for zeros.  Image b reads the source window [pt : h1-pb, pl : w1-pr] (hu x wu) and writes the
 *     destination window [p2t : H2-p2b, p2l : W2-p2r] (h2 x w2); destination pixels outside it are written as 0.  The kernel clamps the
 *     paddings so that hu, wu >= 1 and h2, w2 >= 0 and every source index stays inside [0, h1) x [0, w1) whatever the arrays hold
 *     (callers validate on the host; an empty destination window gives an all-zero image).
 *   planes[0 .. n_planes): src fp32 [B or 1, C, h1, w1] contiguous per image, image b at src + b * src_batch_stride floats (0 broadcasts
 *     one source, e.g. the rays of a single ground-truth camera); mul: optional fp32 [B,1,h1,w1] multiplied into every tap before
 *     blending (points = rays * radius without the product at network resolution); dst fp32 [B,C,H2,W2] contiguous, 4-byte aligned.
 *   Arithmetic along each axis, for window-relative destination index o of n2 from n source samples (fp32, every operation rounded
 *     separately; the same as ud_eval_depth's resample): s = (float)n / (float)n2, f = max(s * ((float)o + 0.5f) - 0.5f, 0),
 *     i0 = min((int)f, n-1), i1 = i0 + (i0 < n-1), l = clamp(f - (float)i0, 0, 1), h = 1 - l;
 *     out = (v00 * hx + v01 * lx) * hy + (v10 * hx + v11 * lx) * ly, every v = src (* mul, rounded) at (y0|y1, x0|x1).
 *     hu == h2 && wu == w2: a bit copy of the window (of the rounded product when mul is given).
 *   Intrinsics (optional, both or neither): K_in, K_out fp32 [B,3,3] (may alias).  With sx = (float)((double)w2 / (double)wu), sy likewise:
 *     fx' = fx * sx, fy' = fy * sy, cx' = (cx - pl) * sx + p2l, cy' = (cy - pt) * sy + p2t, every operation rounded separately; the other
 *     seven entries are copied.  n_planes = 0 with K given runs the intrinsics alone.
 *   Limits: 1 <= B <= 65535, h1, w1, H2, W2 >= 1, C >= 1, C * H2 < 2^31, n_planes <= UD_MATCH_MAX_PLANES; offsets are 64-bit. */
#define UD_MATCH_MAX_PLANES 4
typedef struct UdMatchPlane {
  const float* src; const float* mul; float* dst;
  int C;
  long long src_batch_stride;
} UdMatchPlane;
typedef struct UdMatchGt {
  UdMatchPlane planes[UD_MATCH_MAX_PLANES];
  const int* pads1; const int* pads2;
  const float* K_in; float* K_out;
  int n_planes, B, h1, w1, H2, W2;
} UdMatchGt;
int ud_match_gt(const UdMatchGt* desc, void* stream);

/* ---- output side: maps of a batch rendered as colour images, a grid of panels per image (csrc/colorize.hip) ----
 * The device form of the reference's colorize (unidepth/utils/visualization.py:17-36: numpy + matplotlib, one image per call) and of
 * its image_grid of equal-sized panels (scripts/demo.py: rgb | gt / pred | error), for a whole batch in at most two launches on `stream`
 * (a partial min / max pass only when a panel is auto-ranged, then the render pass): no atomics, no host synchronisation, bitwise
 * reproducible.
 *   dst u8 [B, rows*H, cols*W, 3], or [B, 3, rows*H, cols*W] with UD_CZ_CHW; contiguous, any alignment.  Cell (r, c) is
 *   panels[r * cols + c] and covers dst rows [r*H, (r+1)*H) and columns [c*W, (c+1)*W); rows * cols <= UD_COLORIZE_MAX_PANELS.
 *   Panel kinds (all sources device, contiguous per image; image b at src + b * batch_stride ELEMENTS, so a map may be a channel of a
 *   larger tensor, e.g. depth = points[:, 2]; 0 broadcasts one image):
 *     UD_CZ_NONE  the cell is not written: its bytes keep their bits.
 *     UD_CZ_MAP   src fp32 [H, W]: v = src[y, x].
 *     UD_CZ_AREL  src = g, src2 = p, both fp32 [H, W] (batch_stride2 for p): v = g == 0 ? 0 : fabsf(g - p) / g, every operation rounded
 *                 separately (the demo's error map), then coloured like a map.
 *     UD_CZ_RGB   src u8 [3, H, W] copied through (interleaved for the HWC destination).
 *   Colour of a map value v with the panel's lut u8 [256, 3] (device), in fp32 with IEEE division, every operation rounded separately:
 *     t = (v - lo) / den;  x = t * 256.0f;
 *     x is NaN -> (0,0,0);  x < 0 -> lut[0];  x >= 256 -> lut[255];  otherwise lut[(int)x];  finally v < 1e-4f -> (0,0,0) (false for a NaN).
 *   Range of a panel: without auto flags lo and den are the descriptor's (the host passes lo = (float)vmin and
 *     den = (float)((double)vmax - (double)vmin), numpy's promotion of Python floats against a float32 array; hi is ignored).
 *     UD_CZ_AUTO_LO takes lo = the image's minimum, UD_CZ_AUTO_HI takes hi = its maximum, each over ALL pixels of image b of this panel
 *     (invalid ones included) and NaN if any pixel is NaN, as ndarray.min() / max(); the other limit is the descriptor's lo / hi; then
 *     den = hi - lo rounded in fp32.  The range is per image and per panel.  Flags of an rgb panel are ignored.
 *   work: device scratch of at least ud_colorize_work_bytes(B, H, W) bytes (host-only query: three floats per panel slot and chunk of
 *     1024 pixels), 4-byte aligned, work_bytes its size; needed only when a panel is auto-ranged (NULL otherwise).  No initialisation.
 *   Limits: 1 <= B <= 65535, H, W >= 1, H*W < 2^31, 3*cols*W < 2^31, rows, cols >= 1, rows*cols <= 4, batch strides >= 0, fp32 sources
 *     4-byte aligned; offsets are 64-bit.  The render pass covers a cell with tiles of 4 rows x 256 pixels laid from the 4-byte boundary
 *     at or before a row's first byte, ceil(H / 4) * ceil((W + 3) / 256) of them, and one launch takes at most UD_COLORIZE_MAX_TILES
 *     (its x extent in threads stays below 2^32): this binds only below W = 32, where an image may be 2^26 - 4 rows tall.
 *     ud_colorize_work_bytes answers -1 for sizes beyond these.  Every refusal is returned before any HIP call. */
#define UD_COLORIZE_MAX_PANELS 4
#define UD_COLORIZE_MAX_TILES 0xffffff
enum { UD_CZ_NONE = 0, UD_CZ_MAP = 1, UD_CZ_AREL = 2, UD_CZ_RGB = 3 };
enum { UD_CZ_AUTO_LO = 1, UD_CZ_AUTO_HI = 2 };        /* UdColorPanel.flags */
enum { UD_CZ_CHW = 1 };                               /* UdColorize.flags */
typedef struct UdColorPanel {
  const void* src; const float* src2; const unsigned char* lut;
  long long batch_stride, batch_stride2;
  int kind, flags;
  float lo, hi, den;
} UdColorPanel;
typedef struct UdColorize {
  UdColorPanel panels[UD_COLORIZE_MAX_PANELS];
  unsigned char* dst; void* work; long long work_bytes;
  int B, H, W, rows, cols, flags;
} UdColorize;
int ud_colorize(const UdColorize* desc, void* stream);
long long ud_colorize_work_bytes(int B, int H, int W);

/* ---- output side: the point clouds of a batch splatted into depth maps (csrc/splat.hip) ----
 * The device form of the reference's project_points (unidepth/utils/geometric.py:161-204: a per-image loop of scatter_add_, the mean depth
 * per pixel) and the z-buffer a re-rendered view needs (nearest surface wins), for a whole batch in three plain launches on `stream`
 * (fill the work words, splat one thread per point, resolve one thread per pixel): integer atomics only, no float atomics, no workgroup
 * waiting on another, no host synchronisation.  Bitwise reproducible: the result does not depend on the order the points arrive in.
 *   Sources, all device fp32.  Strided form (offsets == NULL): image b has n_points points; coordinate c of point r is at
 *     xyz[b * batch_stride + r * point_stride + c * comp_stride] (ELEMENTS): planar [B,3,h,w] is (3hw, 1, hw), rows [B,N,3] are (3N, 3, 1);
 *     batch_stride = 0 splats one cloud into every image.  Packed form (offsets != NULL: device int64 [B+1], e.g. UdPointCloud's): n_points
 *     is the number of rows behind xyz, row i is at xyz[i * point_stride + c * comp_stride] (batch_stride is ignored), image b owns the
 *     rows [offsets[b], min(offsets[b+1], n_points)) and r = i - offsets[b]; the kernel finds a row's image by a search over the offsets,
 *     which are never read on the host; rows owned by no image are skipped.  comp_stride = 1 rows are read with one 12-byte load.
 *   Arithmetic per point, fp32, every operation rounded separately, left to right:
 *     T fp32 [nT,3,4] (nT = 1 or B; NULL = none), t = T[b] (T[0] when nT = 1):  x' = ((t00*x + t01*y) + t02*z) + t03, y' and z' likewise
 *       from rows 1 and 2.  Without T: x' = x, y' = y, z' = z.
 *     K fp32 [nK,3,3] (nK = 1 or B; the FULL matrix, as the reference's matmul):  a = (k00*x' + k01*y') + k02*z', b_ and w likewise from
 *       rows 1 and 2;  u = a / w + pixel_offset,  v = b_ / w + pixel_offset  (IEEE division).
 *     Cell: fu = floorf(u), or truncf(u) with UD_SPLAT_TRUNC (the reference's .int(): u in (-1, 0) gives -0.0f and lands in column 0, as
 *       it does there); the column is (int)fu when fu >= 0.0f && fu < 2^31 (decided in float before converting: a NaN or an infinite u
 *       fails, -0.0f passes) and (int)fu < W; otherwise the point is dropped.  Rows likewise from v and H.
 *     UD_SPLAT_RANGE drops the point when !(z' >= dmin && z' <= dmax).  The depth of a point is z'.
 *   mode UD_SPLAT_NEAREST: additionally drops !(z' > 0).  Each kept point makes one 64-bit atomicMin with the key (bits(z') << 32) | r on
 *     its pixel: the smallest z' wins, among equal z' the smallest r.  depth = the winner's z' (its bits), 0 where nothing landed; index
 *     int32 [B,H,W] (optional) = the winner's r, -1 for holes; rgb [B,3,H,W] (with color; u8, or fp32 with color_f32 != 0) = the winner's
 *     colour, gathered from `color` with the SAME strides and offsets as xyz (component = channel), holes 0; count int32 [B,H,W]
 *     (optional; costs a second atomic per point) = the number of kept points on the pixel.
 *   mode UD_SPLAT_MEAN (the reference's semantics; z' <= 0 allowed): drops !(fabsf(z') <= 2^20); each kept point adds llrintf(z' * 2^24)
 *     (round to nearest even; the product is exact) to the pixel's int64 sum and 1 to its uint32 count.
 *     depth = (float)((double)sum / ((double)count * 16777216.0)), 0 where count == 0 and NaN where count >= 2^19 (the sum's headroom);
 *     count int32 [B,H,W] is optional; index and rgb are refused.
 *   outputs: depth fp32 [B,H,W] always; every pixel of every requested output is written, outputs not requested are not touched.
 *   work: device scratch, 8-byte aligned, work_bytes its size: 8 B per pixel of the batch, plus 4 B per pixel when counts are kept (mean
 *     mode, or count given).  ud_splat_work_bytes(B, H, W) (host-only) answers 12 B per pixel, enough for both, and -1 beyond the limits.
 *     Its contents need no initialisation.
 *   Limits: 1 <= B <= 65535, H, W >= 1, H*W < 2^31, 0 <= n_points < 2^31, point_stride, comp_stride >= 1, batch_stride >= 0; offsets are
 *     64-bit.  Every refusal is returned before any HIP call. */
enum { UD_SPLAT_NEAREST = 0, UD_SPLAT_MEAN = 1 };     /* UdSplat.mode */
enum { UD_SPLAT_TRUNC = 1, UD_SPLAT_RANGE = 2 };      /* UdSplat.flags */
typedef struct UdSplat {
  const float* xyz; const long long* offsets; const float* K; const float* T; const void* color;
  float* depth; int* index; void* rgb; int* count;
  void* work; long long work_bytes;
  long long batch_stride, point_stride, comp_stride, n_points;
  int B, H, W, nK, nT, mode, flags, color_f32;
  float pixel_offset, dmin, dmax;
} UdSplat;
int ud_splat(const UdSplat* desc, void* stream);
long long ud_splat_work_bytes(int B, int H, int W);

/* ud_splat with the projection K (x', y', z') replaced by the camera model of the point's image (UdCameraProject's models and parameter
 * rows): the same three launches, work layout (ud_splat_work_bytes), modes, TRUNC / RANGE flags, outputs and packed offsets.
 *   (u, v) = the model's projection of (x', y', z'); the cell comes from u + pixel_offset, v + pixel_offset as in UdSplat.
 *   The depth of a point -- keyed in nearest mode, summed in mean mode, tested by UD_SPLAT_RANGE -- is the model's depth: z', or
 *   |xyz'| for Spherical.  Nearest mode drops !(depth > 0).  In both modes every model but Spherical drops z' <= 0, MEI additionally keeps a
 *   point only if z' + xi |xyz'| > 0, and with UD_SPLAT_FOV a point is kept only if z' >= cos_limit * |xyz'| (the polynomial models fold
 *   points far off the axis back into the image: this is how a caller culls them).
 *   Limits as UdSplat, with 1 <= B <= UD_RECON_MAX_B.  Every refusal is returned before any HIP call. */
enum { UD_SPLAT_FOV = 4 };                            /* UdSplatCamera.flags only, beside UD_SPLAT_TRUNC and UD_SPLAT_RANGE */
typedef struct UdSplatCamera {
  const float* xyz; const long long* offsets; const float* params; const float* T; const void* color;
  float* depth; int* index; void* rgb; int* count;
  void* work; long long work_bytes;
  long long batch_stride, point_stride, comp_stride, n_points;
  int B, H, W, nT, mode, flags, color_f32;
  float pixel_offset, dmin, dmax, cos_limit;
  unsigned char model[UD_RECON_MAX_B];
} UdSplatCamera;
int ud_splat_camera(const UdSplatCamera* desc, void* stream);

/* The reference's `downsample` (unidepth/utils/geometric.py:208-224), a hole-aware min-pool of sparse depth maps, in one launch:
 * src fp32 [N,1,H,W] contiguous -> dst fp32 [N,1,H/factor,W/factor].  Every value == 0 (either sign) of a factor x factor block counts as
 * 1e5f; the output is the block's minimum, written as 0 when it is > 1000, and NaN when the block holds a NaN (torch.min).  Exact.
 * Limits: 1 <= N <= 65535, 1 <= factor <= 64, H and W multiples of factor, H*W < 2^31.  Every refusal is returned before any HIP call. */
typedef struct UdDepthMinPool {
  const float* src; float* dst;
  int N, H, W, factor;
} UdDepthMinPool;
int ud_depth_minpool(const UdDepthMinPool* desc, void* stream);

/* ---- validation inputs: antialiased resize with crop, pad and normalise fused in (csrc/testprep.hip) ----
 * The device form of the reference's test-time ContextCrop (unidepth/datasets/pipelines/transforms.py:1131-1355: crop / zero-pad to a
 * window, TF.resize(BICUBIC, antialias=True) on the uint8 tensor, NEAREST on the validity mask, camera crop and resize) followed by
 * /255 and TF.normalize, and of F.interpolate(mode, antialias=True, align_corners=False) in general: ONE launch on `stream`, no atomics,
 * no workspace, no host synchronisation, bitwise reproducible.
 *   src: [B,C,h,w] contiguous, uint8 (src_u8 = 1) or fp32 (any alignment of its element type).  The window (top, left, height, width)
 *     is in source pixels and may reach outside the image (samples outside are 0, like TF.pad) or cut it.  The window is resized to a
 *     virtual Ho x Wo image of which dst [B,C,Hn,Wn] contiguous holds the rows [dtop, dtop + Hn) and columns [dleft, dleft + Wn)
 *     (Ho = Hn, Wo = Wn, dtop = dleft = 0 for the whole image; a destination window is a resize followed by a crop without the pixels
 *     in between).
 *   Weights along an axis of `in` window samples and `out` virtual destination samples (ATen's _compute_indices_min_size_weights_aa,
 *     align_corners = False), fp32 with every operation rounded separately (the library is built without FMA contraction here):
 *       scale = (float)in / (float)out, big = scale >= 1 ? scale : 1, support = (interp_size * 0.5f) * big (interp_size 4 bicubic, 2
 *       bilinear), inv = scale >= 1 ? 1.0f / scale : 1, center = scale * ((float)i + 0.5f),
 *       xmin = max((int)(center - support + 0.5f), 0), xsize = min((int)(center + support + 0.5f), in) - xmin
 *       (then clamped: 0 <= xmin <= in - 1, 1 <= xsize <= min(in - xmin, UD_RESIZE_MAX_TAPS): no effect inside the limits below),
 *       w_j = filter(((float)(j + xmin) - center + 0.5f) * inv), total = ((w_0 + w_1) + w_2) + ..., w_j = w_j / total.
 *       bicubic (a = -0.5f), x = |x|:  x < 1: ((a + 2) * x - (a + 3)) * x * x + 1;  x < 2: (((x - 5) * x + 8) * x - 4) * a;  else 0.
 *       bilinear (triangle), x = |x|:  x < 1: 1 - x;  else 0.
 *       in == out: xmin = i, xsize = 1, w_0 = 1 (the axis is copied).
 *   Value: the horizontal pass first, t[y][ox] = (w_0 * s[y][xmin]) + w_1 * s[y][xmin + 1] + ... (left to right, products and sums
 *     rounded separately, s = the window's sample as fp32), then the vertical pass over t with the row weights, top to bottom, the same
 *     way.  With both axes copied an fp32 destination is a bit copy of the window.  The result does not depend on the tiling.
 *   out_form: UD_RESIZE_OUT_F32   dst fp32 = the value
 *             UD_RESIZE_OUT_U8    dst uint8 = clamp(rintf(value), 0, 255) (round half to even: what torchvision's resize does to a uint8
 *                                 tensor on a GPU -- cast to float, interpolate, round, clamp, cast)
 *             UD_RESIZE_OUT_NORM  dst fp32 = ((float)u8 / 255.0f - mean[c]) * inv_std[c] of that byte (C <= 4): the reference's resize,
 *                                 /255 and TF.normalize in one store
 *   Mask plane (mask_dst != NULL): uint8 [B,1,Hn,Wn] from mask_src uint8 [B,1,h,w], or from an implied all-ones mask when mask_src is
 *     NULL; cropped / zero-padded by the same window and resized with the NEAREST rule of F.interpolate:
 *     src = min((int)floorf((float)(o + d) * scale), in - 1) along each axis (scale as above, d = dtop / dleft).
 *   Intrinsics (optional, both or neither): K_in, K_out fp32 [B,3,3] (may alias).  camera.crop then camera.resize of a pinhole:
 *     K[0][2] -= (float)left, K[1][2] -= (float)top, then the six entries of the first two rows times zoom = (float)((double)Ho /
 *     (double)height); the third row is copied.  The destination window does not enter.
 *   Limits: B * (C + 1) <= 65535, every size >= 1, height <= UD_RESIZE_MAX_SCALE * Ho and width <= UD_RESIZE_MAX_SCALE * Wo.  A call
 *     beyond the scale limit is REFUSED with UD_ERR_BAD_ARG (the kernel's tiles -- staged span, intermediate rows and the weight tables in
 *     LDS -- are bounded at compile time by UD_RESIZE_MAX_TAPS = 4 * UD_RESIZE_MAX_SCALE + 1 taps; within the bound the host sizes them
 *     for the call's own scale factors; there is no chunked fall-back beyond it).
 *     The kernel clamps every index, so no descriptor content makes it read or write outside its buffers. */
#define UD_RESIZE_BICUBIC 0
#define UD_RESIZE_BILINEAR 1
#define UD_RESIZE_OUT_F32 0
#define UD_RESIZE_OUT_U8 1
#define UD_RESIZE_OUT_NORM 2
#define UD_RESIZE_MAX_SCALE 8
#define UD_RESIZE_MAX_TAPS 33
typedef struct UdResizeAA {
  const void* src; void* dst;
  const unsigned char* mask_src; unsigned char* mask_dst;
  const float* K_in; float* K_out;
  int B, C, h, w;
  int top, left, height, width;
  int Ho, Wo, dtop, dleft, Hn, Wn;
  int src_u8, filter, out_form;
  float mean[4], inv_std[4];
} UdResizeAA;
int ud_resize_aa(const UdResizeAA* desc, void* stream);

/* ---- launch programs: a recorded list of the ops above replayed with one call (host-side runtime) ---- */
typedef struct UdProgram UdProgram;
UdProgram* ud_program_create(void);
void ud_program_destroy(UdProgram*);
int ud_program_size(const UdProgram*);
int ud_program_add_gemm(UdProgram*, const UdGemm*);
int ud_program_add_layernorm(UdProgram*, const UdLayerNorm*);
int ud_program_add_row_stats_finalize(UdProgram*, const float* partials, float* stats, int M, int slabs, int D, float eps);
int ud_program_add_attention(UdProgram*, const UdAttention*);
int ud_program_add_linear_f32(UdProgram*, const UdLinearF32*);
int ud_program_add_camera_head(UdProgram*, const UdCameraHead*);
int ud_program_add_attention_small_f32(UdProgram*, const float* q, const float* kv, float* out, int B, int T, int H, int C, float scale);
int ud_program_add_preprocess(UdProgram*, const UdPreprocess*);
int ud_program_add_fill_rows(UdProgram*, float* dst, const float* src, int n_img, int rows_per_img, int row_off, int D, int ld);
int ud_program_add_camera_intrinsics(UdProgram*, const float* raw, int raw_stride, float* intr4, float* K33, float* Kinv33, float* Kpost33,
                                     int B, int Hn, int Wn, float resize_factor, int pad_l, int pad_t);
int ud_program_add_rays(UdProgram*, const float* Kinv33, float* rays, int nb, int Hn, int Wn, int gt_mode);
int ud_program_add_rays_camera(UdProgram*, const float* params, float* rays, float* scratch, int Hn, int Wn, int model);
int ud_program_add_ray_embed(UdProgram*, const UdRayEmbed*);
int ud_program_add_upsample2x(UdProgram*, const UdUpsample2x*);
int ud_program_add_resize_ac(UdProgram*, const UdResizeAC*);
int ud_program_add_finalize(UdProgram*, const UdFinalize*);
int ud_program_add_nhwc_to_nchw(UdProgram*, const float* in, float* out, int B, int hw, int C, int ld, int rows_per_img);
int ud_program_add_dwconv7(UdProgram*, const UdDwConv7*);
int ud_program_add_layernorm_patchify2(UdProgram*, const float* x, void* out, int B, int H, int W, int C, int ldo, float eps);
int ud_program_add_patchify4(UdProgram*, const float* img, void* out, int B, int H, int W, int ldo);
int ud_program_add_max(UdProgram*, float* dst, const float* src, long long n, int init);
int ud_program_add_spatial_mean(UdProgram*, const float* x, float* out, int B, int HW, int C, int ldo);
int ud_program_add_v1_op(UdProgram*, const UdV1Op*);
/* run ops [first, last) on `stream`; returns 0 or the first failing op's error code.  Stateless: a recorded program is never modified by a replay */
int ud_program_run(const UdProgram*, int first, int last, void* stream);

/* ---- measurement support (bench.py `roofline.attainable_this_box`; not on any inference path): one launch of a pure MFMA instruction stream
 * (v_mfma_f32_32x32x16_f16, 16 independent instructions per iteration and wave, 4 waves per workgroup) on the random fp16 values in `operands`
 * (2 MiB); `sink`: workgroups * 256 floats, never written for finite operands; *flop_out = FLOP of the launch.  What the matrix pipes of this box
 * sustain at their power-limited clock: boxes of one pool differ by several per cent, the datasheet peak (2.5 PFLOP/s) is a constant. */
int ud_calib_mfma_stream(const void* operands, int iters, int workgroups, void* sink, double* flop_out, void* stream);
/* the same for v_mfma_f32_16x16x32_f16 (the GEMM family's instruction): workgroups of 8 waves, sink >= workgroups * 512 floats (round 6) */
int ud_calib_mfma_stream16(const void* operands, int iters, int workgroups, void* sink, double* flop_out, void* stream);

/* library info; ud_struct_size(i): sizeof the i-th descriptor struct in declaration order (UdGemm = 0, UdLayerNorm = 1, UdAttention = 2, UdPreprocess = 3, UdRayEmbed = 4, UdUpsample2x = 5, UdResizeAC = 6, UdFinalize = 7, UdLinearF32 = 8, UdDwConv7 = 9, UdV1Op = 10, UdKnn = 11, UdExtractPatches = 12, UdCameraHead = 13, UdEvalDepth = 14, UdPointCloud = 15, UdMatchGt = 17,
 * UdColorize = 18, UdSplat = 20, UdDepthMinPool = 21, UdResizeAA = 23, UdEval3d = 25, UdReconstruct = 27, UdCameraProject = 28, UdSplatCamera = 29, UdCameraUnproject = 31, UdRemap = 33, UdOverlapMask = 34, UdWarpCamera = 36, UdNormals = 38, UdEvalNormals = 39, UdDepthConsistency = 41, UdTsdfIntegrate = 43, UdTsdfPoints = 44, UdTsdfRender = 45, UdTsdfMesh = 46, UdIcp = 48, UdDepthPyramid = 49; 16, 19, 22, 24, 26, 30, 32, 35, 37, 40, 42 and 47 are not assigned and answer -1 like every unknown
 * index) */
int ud_version(void);
int ud_struct_size(int which);
const char* ud_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
