/* lafs_hip.h -- C ABI of liblafs_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the LAFS
 * data-parallel hot path.
 *
 * The reference (szlbiubiubiu/LAFS_CVPR2024) has no FFI of its own: the hot path sits behind
 * torch.nn.Module objects that dispatch to ATen/cuBLAS/cuDNN.  Each entry point below replaces the
 * implicit device kernels behind one reference call site (cited as file:line, relative to the reference
 * root).  Conventions:
 *   - plain pointers and sizes only (device pointers unless stated), no torch types;
 *   - the CALLER allocates every buffer including workspaces; the library keeps no process-wide device state and reads no
 *     environment variable: the few device objects it needs itself (side streams and events of the trunk passes) and its
 *     kernel-selection options live in a caller-owned per-device context, lafs_ctx (below); calls that share no context and no
 *     buffer are independent (re-entrant per stream);
 *   - every function enqueues work on `stream` and never synchronises the device;
 *   - return value: 0 = success, < 0 = bad argument (see lafs_last_error()), > 0 = hipError_t;
 *   - "bf16" = raw 16-bit bfloat16, "f32" = IEEE float; row-major everywhere, ld* in ELEMENTS.
 */
#ifndef LAFS_HIP_H
#define LAFS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#define LAFS_ABI_VERSION 1

int lafs_version(void);
/* Diagnostic: lane l of one wave issues ds_read_b64_tr_b16 at LDS byte 8*l over in(i16)[512]; out(i16)[256] gets
 * the 4 values each lane received.  Pins the LDS-transpose-read model used by the attention / wgrad kernels. */
int lafs_debug_tr16(const void* in, void* out, hipStream_t stream);
/* Debug flags: lafs_debug_set records a value and lafs_debug_get returns it; no kernel or dispatch reads it.  bench.py refuses to
 * run unless lafs_debug_get() == 0.  lafs_ablation_build() returns 0: there is no ablation build of this library. */
int lafs_debug_set(int flags);
int lafs_debug_get(void);
int lafs_ablation_build(void);
/* Thread-local text of the last error returned on this thread ("" if none). */
const char* lafs_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Per-device context.  The reference has no counterpart: its modules issue every op on torch's current stream from one Python
 * thread per rank (lafs_train.py:513-613).  This library forks a trunk pass over side streams of its own (row chains, weight
 * gradients), so it needs streams / events that live across calls; they belong to a handle the CALLER creates and destroys.
 *   lafs_ctx_create(device)  device < 0 = the current one.  Creates three non-blocking side streams, their fork / join events and a
 *                            pool of 64 events now (never inside a hipGraph capture); NULL on failure (lafs_last_error()).
 *   lafs_ctx_destroy         after every graph that captured work of this context has been destroyed.
 *   lafs_ctx_set / _get      kernel-selection options (defaults = the measured-best settings; the others exist for A/B runs).
 * A NULL context is legal wherever one is accepted: compiled-in default options, no side streams (everything on `stream`).
 * Two contexts share nothing: engines built on different contexts may be driven from different host threads and streams. */
typedef struct lafs_ctx lafs_ctx;
enum {
  LAFS_OPT_SIDE_STREAMS = 0,   /* 1: row chains / attention groups / weight gradients may use the context's side streams; 0: caller's stream only */
  LAFS_OPT_ROW_CHAINS = 1,     /* 1, 2 (default) or 4 chains of launches over the crop-resolution groups' rows (csrc/engine.hip) */
  LAFS_OPT_KRES_MASK = 2,      /* epilogues routed to the K-resident GEMM: 1 plain, 2 GELU, 4 residual, 8 GELU' (default 15) */
  LAFS_OPT_KRES_MIN_ITEMS = 3, /* accepted and unused: the K-resident GEMM's runs are no longer bounded from below (kres_partition, csrc/gemm_kres.hip) */
  LAFS_OPT_NT_WIDE = 4,        /* tiled GEMM: 128x384 tiles where they fit one round of the chip (default 1) */
  LAFS_OPT_NT_TALL = 5,        /* tiled GEMM: 160-row tiles where they save a round of workgroup slots (default 1) */
  LAFS_OPT_COMM_CUS = 6,       /* data-parallel runs: CUs left to the collective library's kernels by the K-resident GEMM (default 0) */
  LAFS_OPT_NT_BIG = 7,         /* tiled GEMM: one-workgroup-per-CU 192x256 / 176x256 tiles for the wide long-K shapes (default 1; 2-4 force a geometry) */
  LAFS_OPT_MLP_FUSED = 8,      /* trunk passes: the block's MLP as ONE launch (lafs_mlp_fused) where it applies (dim 384, no element dropout):
                                  a mask of LAFS_MLP_FUSED_* bits (default LAFS_MLP_FUSED_DEFAULT); lafs_trunk_plan reports what they come to */
  LAFS_OPT_COUNT = 9
};
enum {                                 /* bits of LAFS_OPT_MLP_FUSED */
  LAFS_MLP_FUSED_FWD = 1,              /* the forward-only pass runs fc1 -> GELU -> fc2 -> residual as one launch */
  LAFS_MLP_FUSED_FWD_SAVE = 2,         /* the saving forward does, and writes gelu'(u) and gelu(u) for the backward */
  LAFS_MLP_FUSED_BWD = 4,              /* the backward's two MLP input-gradient GEMMs are one launch */
  LAFS_MLP_FUSED_LN2 = 8,              /* LayerNorm 2 inside the fused forward (no launch, no round trip of its output) */
  LAFS_MLP_FUSED_LN2_BWD = 16,         /* LayerNorm 2's backward inside the fused backward */
  LAFS_MLP_FUSED_MERGE_CHAINS = 32,    /* (lab) the row chains meet in front of every MLP: one launch over all rows; switches NEXT_LN1 off */
  LAFS_MLP_FUSED_NEXT_LN1 = 64,        /* the fused forward also writes the NEXT block's LayerNorm 1 (bit-identical to its launch) */
  LAFS_MLP_FUSED_PROJ_FWD = 128,       /* forward-only pass: the attention branch's output projection + residual in FRONT of the fused forward */
  LAFS_MLP_FUSED_PROJ_FWD_SAVE = 256,  /* the same in the saving forward (both need LN2 and inner == dim) */
  LAFS_MLP_FUSED_DEFAULT = 1 + 2 + 4 + 8 + 64   /* = 79: step A/B in DESIGN.md section 6 */
};
lafs_ctx* lafs_ctx_create(int device);
void lafs_ctx_destroy(lafs_ctx* ctx);
int lafs_ctx_set(lafs_ctx* ctx, int opt, int value);
int lafs_ctx_get(const lafs_ctx* ctx, int opt);

/* ------------------------------------------------------------------------------------------------
 * GEMMs (nn.Linear / nn.Conv2d(k=s=p) forward, dgrad, wgrad)
 *   vision_transformer.py:59-65 (Mlp), :75-90 (qkv/proj), :126-131 (PatchEmbed conv), :295-301 (DINOHead)
 *   face_pre_pro/ViT_face.py:126-137 (FeedForward), :147-149 (to_qkv/to_out), :761 (patch_to_embedding)
 * ------------------------------------------------------------------------------------------------ */
enum {
  LAFS_EPI_BF16 = 0,       /* C(bf16) = acc + bias                                                   */
  LAFS_EPI_BF16_GELU = 1,  /* C(bf16) = u = acc + bias (skipped when C is NULL) ; C2(bf16) = GELU_erf(u) */
  LAFS_EPI_RESID_F32 = 2,  /* C(f32) = resid + seq_scale[row2seq[m]] * (acc + bias)   (DropPath)     */
  LAFS_EPI_F32 = 3,        /* C(f32) = acc + bias                                                    */
  LAFS_EPI_DGELU_BF16 = 4, /* C(bf16) = acc * GELU'(aux[m][n])                                       */
  LAFS_EPI_ATOMIC_F32 = 5, /* C(f32) += acc, K split into `splits` slices (C must be pre-zeroed)     */
                           /* (LAFS_EPI_F32 with splits > 1: C is [splits][M][ldc], one plain-store image per K slice, no bias;
                            *  lafs_sum_slices adds them -- no atomics, deterministic) */
  LAFS_EPI_EMBED_F32 = 6,  /* C(f32)[m + m/npatch + 1] = acc + bias + pos[1 + m%npatch]  (tokens)    */
  LAFS_EPI_BF16_ACT = 7    /* C(bf16) = act(acc + bias + aux[m][n])   (aux bf16 residual or NULL)    */
};

enum { LAFS_ACT_NONE = 0, LAFS_ACT_RELU = 1, LAFS_ACT_HSWISH = 2, LAFS_ACT_HSIGMOID = 3 };

typedef struct lafs_gemm_nt_args {
  const void* A; int lda;          /* bf16 [M, K]                                  */
  const void* B; int ldb;          /* bf16 [N, K]  (nn.Linear weight layout)       */
  int M, N, K;                     /* K % 32 == 0                                  */
  int epilogue;                    /* LAFS_EPI_*                                   */
  void* C; int ldc;                /* bf16 or f32 [M, N]                           */
  void* C2; int ldc2;              /* second output (BF16_GELU)                    */
  const float* bias;               /* f32 [N] or NULL                              */
  const float* resid; int ldr;     /* f32 [M, N] (RESID_F32; may alias C)          */
  const float* seq_scale;          /* f32 [n_seq] or NULL (RESID_F32)              */
  const int32_t* row2seq;          /* i32 [M]  row -> sequence index               */
  const void* aux; int ldaux;      /* bf16 [M, N] pre-activation (DGELU_BF16)      */
  const float* pos; int npatch;    /* f32 [npatch+1, N] (EMBED_F32)                */
  int splits;                      /* ATOMIC_F32 / F32: number of K slices (>=1)   */
  float drop_p; uint32_t drop_seed; /* element dropout (0 = off): on the linear's output before the residual add
                                      (RESID_F32), on GELU(u) (BF16_GELU: C2 only), and its backward (DGELU_BF16).
                                      Counter-based mask of (drop_seed, row, col): see lafs_debug_dropout_mask.       */
  const float* drop_step;          /* NULL, or DEVICE pointer to the step counter: the mask's seed is drop_seed + 7919 * step, read
                                      when the kernel runs -- a captured hipGraph then draws a new mask on every replay            */
  int drop_row0;                   /* this launch's row 0 is row drop_row0 of the mask (a launch over a row sub-range of a batch) */
  int act;                         /* BF16_ACT: LAFS_ACT_*.  BF16_GELU / DGELU_BF16: LAFS_GELU_SAVE_GRAD (see below) */
  int operand_f16;                 /* 1: A, B, a 16-bit C and the BF16_ACT residual (aux) are IEEE fp16 instead of bf16 (BF16 / BF16_ACT /
                                      F32 epilogues, no K split): the trainable landmark CNN runs in the reference's autocast
                                      format (train_largescale.py:803-804; v_mfma_f32_16x16x32_f16, same rate) */
  const lafs_ctx* ctx;             /* kernel-selection options (NULL = defaults) */
} lafs_gemm_nt_args;

/* act = LAFS_GELU_SAVE_GRAD with LAFS_EPI_BF16_GELU: C receives gelu'(u) (bf16) instead of the pre-activation u; with
 * LAFS_EPI_DGELU_BF16: aux holds that gelu'(u) and is multiplied in as it is.  The backward of Mlp (vision_transformer.py:59-65)
 * needs u only through gelu'(u): saved this way, the derivative's exponential / reciprocal are the forward's (shared with
 * gelu(u)) and the GELU' epilogue of the input gradient is one multiply per value. */
#define LAFS_GELU_SAVE_GRAD 1
/* Number of K slices a request for `splits` actually produces (slices are whole pipeline stages): the image count of a
 * K-split LAFS_EPI_F32 GEMM. */
int lafs_gemm_nt_slices(int K, int splits);
/* C[M,N] = A[M,K] * B[N,K]^T with a fused epilogue.
 * Shape and alignment contract (a request that breaks it returns a negative code and launches nothing):
 *   - K % 32 == 0.  N is free: it need NOT be a multiple of 8 (or of 4 for the fp32 outputs); the last, partial column group of a row
 *     is read and written element by element, and nothing between column N and the row stride is touched.
 *   - A, B: 16-byte aligned, lda % 8 == 0, ldb % 8 == 0 (16-byte row pieces).
 *   - C: 16-byte aligned and ldc % 8 == 0 for every epilogue but ATOMIC_F32 (element-wise atomics: ldc % 8 == 0 only).
 *   - C2 (BF16_GELU): 16-byte aligned, ldc2 % 8 == 0.
 *   - resid (RESID_F32): 16-byte aligned, ldr % 4 == 0 (one 16-byte load per group of 4 columns); it may alias C.
 *   - aux of DGELU_BF16: 16-byte aligned, ldaux % 8 == 0 (one 16-byte load per group of 8 columns).
 *     aux of BF16_ACT is read element by element: any ldaux >= N.
 *   - bias, pos, seq_scale, row2seq: element-aligned.
 * A column slice of a wider buffer is therefore a legal operand when it starts at a multiple of 8 elements (16-bit) / 4 elements
 * (fp32) of a 16-byte aligned row. */
int lafs_gemm_nt(const lafs_gemm_nt_args* args, hipStream_t stream);
/* Which kernel lafs_gemm_nt runs for this request: 0 = the tiled LDS-DMA kernel (gemm.hip), 1 = the K-resident streaming kernel
 * (gemm_kres.hip: K == 384, N % 64 == 0, N <= 1536, M >= 2048, plain / GELU / GELU' / residual epilogue, no dropout, bf16 operands),
 * 3 = the tiled kernel in its 128x384 / 12-wave form (whole N per workgroup: long reductions onto N = 384 whose tiles fit one
 * round of the chip), 4 = the tiled kernel with 160-row tiles (long reductions whose 128-row tiles would spill into one more
 * round of the 512 workgroup slots than 160-row ones need), 5 = the 256x256 one-workgroup-per-CU kernel (gemm_big.hip).
 * This is lafs_gemm_nt's own decision, not a restatement of it: both run the same plan.  A request lafs_gemm_nt refuses -- for
 * any reason: a null operand, K % 32, alignment, the fp16 rule, the dropout ranges, a missing epilogue operand, a biased K split --
 * gives the same negative code here, not a route, and sets lafs_last_error().  No device is needed and nothing is dereferenced. */
int lafs_gemm_nt_route(const lafs_gemm_nt_args* args);
/* The whole plan of a request, from the same call: what lafs_gemm_nt would launch.  Returns 0 and fills *out, or the negative code
 * lafs_gemm_nt would return (then *out is untouched).
 *   route            as lafs_gemm_nt_route
 *   tile_m, tile_n   output rows x columns of a workgroup's tile (tiled kernel: 128 / 160 / 256 x 128 / 384; K-resident: one work
 *                    item, 128 x 64; one-workgroup-per-CU kernel: 160 / 176 / 192 / 256 x 256)
 *   stage_k          k-depth of a pipeline stage (32 or 64; K-resident: 384, a stage holds weight rows over the whole K)
 *   threads          threads per workgroup
 *   f16              1: the fp16 instantiation (operand_f16)
 *   k_slices         K slices (> 1 only for ATOMIC_F32 / F32 with splits: lafs_gemm_nt_slices)
 *   workgroups       workgroups launched, over all K slices */
typedef struct lafs_gemm_nt_plan_info {
  int route, tile_m, tile_n, stage_k, threads, f16, k_slices, workgroups;
} lafs_gemm_nt_plan_info;
int lafs_gemm_nt_plan(const lafs_gemm_nt_args* args, lafs_gemm_nt_plan_info* out);

/* ------------------------------------------------------------------------------------------------
 * Fused MLP of a ViT-S block (csrc/mlp_fused.hip): two chained GEMMs, the hidden-wide intermediate never leaves the chip.
 *   vision_transformer.py:59-65 (Mlp.forward: fc1 -> GELU -> fc2) with the residual + DropPath of Block.forward (:112), and the
 *   input-gradient chain of the same lines in the backward.  Embedding width 384 (compile time), hidden width H % 64 == 0,
 *   128 <= H <= 1536.  Results are bit-identical to the two lafs_gemm_nt launches each mode replaces.
 *   LAFS_MLP_FWD       out(f32)[M,384] = resid + seq_scale[row2seq[m]] * (gelu(X Wa^T + bias_a) Wb^T + bias_b)
 *                      X = LayerNorm-2 output (bf16), Wa = fc1.weight [H,384], Wb = fc2.weight [384,H] (bf16 shadows);
 *                      replaces lafs_gemm_nt(LAFS_EPI_BF16_GELU, C == NULL) + lafs_gemm_nt(LAFS_EPI_RESID_F32)
 *   LAFS_MLP_FWD_SAVE  the same, and save_grad(bf16)[M,H] = gelu'(u), save_act(bf16)[M,H] = gelu(u) are written (what the backward
 *                      and the fc2 weight gradient read): replaces (LAFS_EPI_BF16_GELU, act = LAFS_GELU_SAVE_GRAD) + RESID_F32
 *   LAFS_MLP_BWD       save_act(bf16)[M,H] = du = (X Wa^T) * save_grad  (written: the fc1 weight gradient's operand),
 *                      out(bf16)[M,384] = du Wb^T;  X = upstream gradient (bf16), Wa = fc2.weight^T shadow [H,384],
 *                      Wb = fc1.weight^T shadow [384,H]: replaces (LAFS_EPI_DGELU_BF16, act = LAFS_GELU_SAVE_GRAD) + LAFS_EPI_BF16
 * One 8-wave workgroup per 128 rows (rows past the last full round of the chip: 64-row units); caller-allocated buffers only;
 * never synchronises. */
enum { LAFS_MLP_FWD = 0, LAFS_MLP_FWD_SAVE = 1, LAFS_MLP_BWD = 2 };
typedef struct lafs_mlp_args {
  const void* X; int ldx;          /* bf16 [M, 384]                                       */
  const void* Wa; int ldwa;        /* bf16 [H, 384]                                       */
  const void* Wb; int ldwb;        /* bf16 [384, H]                                       */
  int M, H;
  int mode;                        /* LAFS_MLP_*                                          */
  const float* bias_a;             /* f32 [H]   or NULL (forward modes)                   */
  const float* bias_b;             /* f32 [384] or NULL (forward modes)                   */
  const float* resid; int ldr;     /* f32 [M, 384] (forward modes; may alias out)         */
  const float* seq_scale;          /* f32 [n_seq] or NULL (forward modes: DropPath)       */
  const int32_t* row2seq;          /* i32 [M]                                             */
  void* out; int ldo;              /* f32 [M, 384] (forward) / bf16 [M, 384] (backward)   */
  void* save_grad; int ldsg;       /* bf16 [M, H]: gelu'(u), written by FWD_SAVE, read by BWD */
  void* save_act; int ldsa;        /* bf16 [M, H]: FWD_SAVE writes gelu(u); BWD writes du */
  const lafs_ctx* ctx;             /* rounds of the chip are sized by the context's CU count (NULL: one launch of 128-row units) */
  /* LayerNorm prologue (forward modes; vision_transformer.py:112 `self.norm2`): with ln_gamma != NULL, X is ignored and the GEMM-1
   * operand is LayerNorm(resid; ln_gamma, ln_beta, ln_eps) computed inside the kernel, bit-identical to lafs_layernorm_fwd on
   * >= 4096 rows; ln_stats (f32 [M, 2]: mean, rstd) and ln_out (bf16 [M, 384]: the operand itself -- what the LayerNorm backward
   * and the fc1 weight gradient read) are written when not NULL. */
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  float* ln_stats; void* ln_out; int ldln;
  /* LayerNorm backward in the epilogue (LAFS_MLP_BWD with ln_gamma != NULL): out is not written; instead, with x = resid (f32
   * [M, 384]) and its statistics ln_stats (read), dx = LN'(bf16(dX)) is added into ln_g_io (f32 [M, 384], the residual gradient
   * stream), ln_gb_out (bf16 [M, 384]) = bf16(seq_scale[row2seq[m]] * ln_g_io) and the launch's gamma / beta sums go to
   * ln_part_out (f32 [lafs_mlp_fused_ln_parts(M)][2][384], the slot layout of lafs_layernorm_bwd: fold with
   * lafs_layernorm_bwd_fold) -- what lafs_layernorm_bwd(accumulate = 1) computes from the stored dX, without the launch. */
  float* ln_g_io; int ldgio; void* ln_gb_out; int ldgb; float* ln_part_out;
  /* The NEXT block's LayerNorm 1 in the epilogue (forward modes; vision_transformer.py:110 `self.norm1` of block l + 1): with
   * next_ln_gamma != NULL the finished rows of `out` are normalised where they sit in registers -- next_ln_out (bf16 [M, 384]) =
   * LayerNorm(out; next_ln_gamma, next_ln_beta, next_ln_eps), next_ln_stats (f32 [M, 2], may be NULL) = (mean, rstd) -- what
   * lafs_layernorm_fwd on `out` computes, bit for bit at >= 4096 rows (the summation order of its two-rows-per-wave kernel is repeated). */
  const float* next_ln_gamma; const float* next_ln_beta; float next_ln_eps;
  float* next_ln_stats; void* next_ln_out; int ldnln_next;
  /* The attention branch's output projection in FRONT (forward modes with ln_gamma != NULL; vision_transformer.py:88-90 `self.proj`
   * and the residual / DropPath of Block.forward :111): with proj_x != NULL (bf16 [M, 384], the attention output) the kernel first
   * computes  resid = proj_resid + proj_scale[row2seq[m]] * (proj_x proj_w^T + proj_bias)  -- `resid` (fp32 [M, 384]) is then an
   * OUTPUT, written once, normalised from registers (LayerNorm 2) and read back by the final epilogue as the residual; proj_w bf16
   * [384, 384] row-major (out, in), proj_bias fp32 [384] or NULL, proj_resid fp32 [M, 384], proj_scale per sequence or NULL.
   * Replaces lafs_gemm_nt(LAFS_EPI_RESID_F32) of the projection, bit for bit where that call runs on the K-resident kernel. */
  const void* proj_x; int ldpx; const void* proj_w; int ldpw; const float* proj_bias;
  const float* proj_resid; int ldpr; const float* proj_scale;
} lafs_mlp_args;
int lafs_mlp_fused(const lafs_mlp_args* args, hipStream_t stream);
/* Slots a LAFS_MLP_BWD launch with the LayerNorm epilogue writes for M rows (one per 128-row workgroup). */
int lafs_mlp_fused_ln_parts(int rows);
/* 1 when lafs_mlp_fused takes this geometry (dim == 384, hidden % 64 == 0 in [128, 1536]), else 0. */
int lafs_mlp_fused_supported(int dim, int hidden, int rows);

/* C[N1,N2] (f32) += A[M,N1]^T * B[M,N2]   (weight gradient dW = dY^T X; reduction over the token axis,
 * split over `splits` workgroups with fp32 atomics; splits <= 0 picks a default).  N1,N2,lda,ldb % 8 == 0.
 * colsum_a (optional f32 [N1]) += column sums of A: the bias gradient db = sum_m dY[m,:] rides along for free. */
int lafs_gemm_tn_acc(const void* A, int lda, const void* B, int ldb, float* C, int ldc,
                     int M, int N1, int N2, int splits, float* colsum_a, hipStream_t stream);
/* Same contraction, accumulated into per-XCD images: part(f32) [LAFS_N_XCD][...], image x at part + x*part_stride.  Every
 * XCD adds into its own image with L2-local atomics (no cross-XCD traffic); fold with lafs_reduce_partials.  The images must
 * be zero before the first accumulation (lafs_reduce_partials leaves them zeroed). */
int lafs_gemm_tn_part(const void* A, int lda, const void* B, int ldb, float* part, int ldc, int64_t part_stride,
                      int M, int N1, int N2, int splits, float* colsum_a, hipStream_t stream);
/* out(f32)[i] += sum_x part[x*part_stride + i], then part[...] = 0;  n, part_stride multiples of 4; part and out 16-byte aligned
 * (float4 loads and stores; likewise lafs_sum_slices) -- anything else is refused with a negative code. */
int lafs_reduce_partials(float* part, int64_t part_stride, int n_part, int64_t n, float* out, hipStream_t stream);
/* out(f32)[n] = sum over x < n_part of part[x * part_stride + i]: folds the slice images of a K-split LAFS_EPI_F32 GEMM. */
int lafs_sum_slices(const float* part, int64_t part_stride, int n_part, int64_t n, float* out, hipStream_t stream);

/* Second-generation weight gradient (csrc/wgrad.hip): C[N1,N2] = (accumulate ? C : 0) + A[M,N1]^T * B[M,N2].
 * One 4-wave workgroup per CU (one wave per SIMD, 512 registers) owns a (64 FA) x (64 FB) tile of v_mfma_f32_32x32x16_bf16
 * blocks (192x192 .. 256x256) over one slice of the token axis and STORES its fp32 tile into `workspace`
 * ([slices][N1][N2] f32 per GEMM); a fold kernel then writes C: no atomics, and with accumulate = 0 the gradient buffer needs
 * no memset.  colsum_a (f32 [N1]) += column sums of A: every (slice, tile, wave column) stores its share into the workspace and
 * the fold kernel adds the shares in a fixed order (deterministic; fp32 atomics before round 5).
 * lafs_wgrad_group runs up to 8 such GEMMs that share the token count M (the four weight gradients of one transformer block)
 * as ONE launch + ONE fold: the tiles of all GEMMs fill the chip together, so the token axis is cut into 4x fewer slices --
 * 4x less partial-sum traffic, 4x longer main loops per workgroup.
 * Calls that share a workspace must be ordered on one stream.  N1, N2, lda, ldb % 8 == 0, ldc % 4 == 0. */
typedef struct lafs_wgrad_item {
  const void* A; int lda;          /* bf16 [M, N1]  (dY)                            */
  const void* B; int ldb;          /* bf16 [M, N2]  (X)                             */
  float* C; int ldc;               /* f32 [N1, N2]  (dW)                            */
  int N1, N2;
  int accumulate;                  /* 0: C = A^T B ; 1: C += A^T B                  */
  float* colsum_a;                 /* f32 [N1] += column sums of A (bias gradient), or NULL */
} lafs_wgrad_item;
/* max_workgroups: how many workgroups (= CUs) the launch may occupy, 8..256; 0 = the whole chip.  A backward pass that runs
 * its weight gradients on a side stream keeps part of the chip free for the HBM-bound kernels of the main stream this way
 * (the LAFS step: 160 of 256, 18.8 -> 18.5 ms).  The workspace size depends on it. */
int64_t lafs_wgrad_group_workspace_bytes(const lafs_wgrad_item* items, int n_items, int M, int max_workgroups);
int lafs_wgrad_group(const lafs_wgrad_item* items, int n_items, int M, int max_workgroups, void* workspace,
                     int64_t workspace_bytes, hipStream_t stream);
int64_t lafs_wgrad_workspace_bytes(int M, int N1, int N2);
/* lafs_wgrad with fp16 operands (the landmark CNN's activations and activation gradients, see lafs_gemm_nt_args::operand_f16). */
int lafs_wgrad_f16(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N1, int N2,
                   int accumulate, float* colsum_a, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int lafs_wgrad(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N1, int N2,
               int accumulate, float* colsum_a, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* out(f32)[n] += sum_m X(bf16)[m, n]   (bias gradients). */
int lafs_colsum_bf16_acc(const void* X, int ldx, int M, int N, float* out, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm  (vision_transformer.py:99,103,156 eps 1e-6; face_pre_pro/ViT_face.py:117 eps 1e-5)
 * ------------------------------------------------------------------------------------------------ */
/* y(bf16)[r,:] = (x(f32)[r,:] - mean) * rstd * gamma + beta ; stats(f32)[r] = {mean, rstd}.
 * y_f32 (optional, may be NULL) receives the same result in fp32.  D % 4 == 0, D <= 2048; ldx, ldy, ldyf multiples of 4. */
int lafs_layernorm_fwd(const float* x, int ldx, const float* gamma, const float* beta, float eps,
                       void* y_bf16, int ldy, float* y_f32, int ldyf, float* stats, int rows, int D,
                       hipStream_t stream);
/* Backward.  dy is bf16 [rows, D] (dy_f32 != NULL: use that fp32 gradient instead).
 *   dx = LN'(dy);  g_io(f32)[r,:] = (accumulate ? g_io : 0) + dx
 *   dgamma(f32)[D] += sum_r dy*xhat ; dbeta(f32)[D] += sum_r dy
 *   gb_out(bf16, optional)[r,:] = bf16(seq_scale[row2seq[r]] * g_io[r,:])  -- the DropPath-scaled gradient fed to
 *   the previous residual branch's GEMMs (seq_scale NULL -> scale 1).
 * Row strides of the operands in use -- ldx, ldg, lddyf (with dy_f32) or lddy (without), ldgb (with gb_out) -- must be multiples
 * of 4, as for the forward (vector loads and stores); anything else is refused (LAFS_ESHAPE). */
int lafs_layernorm_bwd(const void* dy_bf16, int lddy, const float* dy_f32, int lddyf, const float* x, int ldx,
                       const float* stats, const float* gamma, float* g_io, int ldg, int accumulate,
                       void* gb_out, int ldgb, const float* seq_scale, const int32_t* row2seq,
                       float* dgamma, float* dbeta, int rows, int D, float drop_p, uint32_t drop_seed,
                       const float* drop_step, int drop_row0, float* part_out, hipStream_t stream);
/* Deterministic parameter gradients: with part_out != NULL (f32 [lafs_layernorm_bwd_parts(rows, D)][2][D]) the launch stores every
 * workgroup's gamma / beta sums into a slot of its own and leaves dgamma / dbeta alone (they may be NULL);
 * lafs_layernorm_bwd_fold then adds the slots of up to 4 launches per LayerNorm (the row chains of a trunk pass) in a fixed order:
 * dgamma[c] += sum, dbeta[c] += sum.  Without part_out the sums leave as one fp32 atomic per column and workgroup. */
#define LAFS_LN_FOLD_MAX 24
typedef struct lafs_ln_fold_item {
  const float* part[4]; int n_parts[4];      /* unused entries: NULL / 0 */
  float* dgamma; float* dbeta;
} lafs_ln_fold_item;
int lafs_layernorm_bwd_parts(int rows, int D);
int lafs_layernorm_bwd_fold(const lafs_ln_fold_item* items, int n_items, int D, hipStream_t stream);

/* gb(bf16)[r,:] = bf16(seq_scale[row2seq[r]] * g(f32)[r,:])  (seq_scale NULL -> plain cast).  D, ldg and ldgb must be multiples of 4. */
int lafs_scale_cast_bf16(const float* g, int ldg, void* gb, int ldgb, const float* seq_scale,
                         const int32_t* row2seq, int rows, int D,
                         float drop_p, uint32_t drop_seed, const float* drop_step, int drop_row0, hipStream_t stream);
/* Element dropout (nn.Dropout of Part-fViT, face_pre_pro/ViT_face.py:131-133,150-153,614).  The mask is a pure function
 * of (drop_seed, row, col, n_cols): factor(r,c) = mix32(r*n_cols + c, seed) >= drop_p*2^32 ? 1/(1-drop_p) : 0, so a
 * backward kernel regenerates the forward's mask from the same seed; drop_p = 0 disables it.  In lafs_layernorm_bwd and
 * lafs_scale_cast_bf16 the factor multiplies gb_out (the gradient entering a dropped-out branch output).
 * lafs_dropout_f32: x(f32)[rows, D] *= factor in place (embedding dropout, forward and backward).
 * lafs_debug_dropout_mask: out(f32)[rows, cols] = factor (tests feed it to the oracle).
 * drop_step (NULL or a DEVICE pointer to a float step counter): the seed used is drop_seed + 7919 * (uint32)step, read when the
 * kernel runs, so a hipGraph-captured training step draws new masks on every replay (reference: nn.Dropout draws per call);
 * drop_row0: the launch covers rows [drop_row0, drop_row0 + rows) of the mask (row chains of the trunk passes).  A host-side
 * seed' = drop_seed + 7919 * step with drop_step = NULL produces the identical mask. */
int lafs_dropout_f32(float* x, int ldx, int rows, int D, float drop_p, uint32_t drop_seed, const float* drop_step, hipStream_t stream);
int lafs_debug_dropout_mask(int rows, int cols, float drop_p, uint32_t drop_seed, float* out, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused multi-head attention over variable-length sequences, head_dim = 64
 *   vision_transformer.py:80-89 (scale = head_dim^-0.5); face_pre_pro/ViT_face.py:155-179 (scale = dim^-0.5)
 * qkv(bf16) [T, 3*H*64]: columns [q | k | v], each H*64 wide, head-major.  cu_seqlens(i32, device) [n_seq+1].
 * All sequences of one call must have length <= max_len <= 256.  cu_seqlens is read through the scalar (constant) cache: it must not
 * be written while a launch that reads it is in flight (the engines build it once per geometry).
 * ------------------------------------------------------------------------------------------------ */
int lafs_attention_fwd(const void* qkv, int ldqkv, const int32_t* cu_seqlens, int n_seq, int max_len, int heads,
                       float scale, void* out_bf16, int ldo, float* lse, hipStream_t stream);
/* dqkv(bf16) [T, 3*H*64] from dout(bf16) [T, H*64], out(bf16) and lse(f32) [T, H] of the forward: one launch per call (Q, K, V,
 * dO of a (sequence, head) staged once; delta = rowsum(dO * O) formed on the way in).
 * Padded positions (the tiles are 16 rows; a sequence's last tile and the tiles up to max_len's dispatch class are padding): both
 * entry points write exactly the rows of the T tokens and the columns of their H*64 (3*H*64) channels, nothing else, and a padded
 * position never contributes to a stored value, whatever the logits: padded keys are excluded from the forward's maximum and sum
 * and from dQ (their weight against a real query would be exp(-lse), which overflows for lse < -88.7), padded queries carry
 * dO = 0, Q = 0.  Finite inputs with finite fp32 logits give finite outputs for every lse a row can have. */
int lafs_attention_bwd(const void* qkv, int ldqkv, const void* out_bf16, int ldo, const void* dout_bf16, int lddo,
                       const float* lse, const int32_t* cu_seqlens, int n_seq, int max_len, int heads, float scale,
                       void* dqkv, int lddqkv, hipStream_t stream);
/* The attention probabilities themselves, for inspection (vision_transformer.py:85-86 `attn`, returned by get_last_selfattention;
 * face_pre_pro/ViT_face.py:165,175-177 `attention_score`): probs(f32) [n_seq, H, nq, max_len], nq = q_rows > 0 ? q_rows : max_len,
 * row (s, h, i, :) = softmax_j(scale * q_i . k_j) over the len_s keys of sequence s.  Key columns j >= len_s and query rows i >= len_s
 * are written as exact zeros (the buffer needs no clearing); q_rows = 1 is the cls-query form (attn[:, :, 0, :]) and costs one query
 * tile per (sequence, head).  The scores are formed as lafs_attention_fwd forms them (bf16 operands, fp32 accumulation, exp2 of the
 * scale * log2(e)-folded scores, fp32 maximum / sum / normalisation); P is not rounded to bf16 and the forward's lse is not needed. */
int lafs_attention_probs(const void* qkv, int ldqkv, const int32_t* cu_seqlens, int n_seq, int max_len, int heads,
                         float scale, int q_rows, float* probs, hipStream_t stream);
/* Attention of the cls query alone (the last block of a trunk whose output is read through x[:, 0], vision_transformer.py:209-215): for
 * every (sequence s, head h) query row 0 of the sequence against its len_s keys.  Row s of the COMPACT outputs belongs to sequence s of
 * the call: out_c(bf16) [n_seq, ldo >= H*64], lse_c(f32) [n_seq, H] (natural log-sum-exp of the scaled scores).  Plain fp32 arithmetic
 * on the bf16 operands -- scores, maximum, sum and P V in fp32 -- with the un-normalised P rounded to bf16 in front of P V and the
 * normaliser summed from the unrounded P, exactly where lafs_attention_fwd rounds: the two forwards differ by fp32 summation order
 * only.  16 bits are STORED exactly once: out_c.
 * Reads only the q columns of the first row and the k | v columns of every row of the call's sequences; lengths 1..256. */
int lafs_attention_cls_fwd(const void* qkv, int ldqkv, const int32_t* cu_seqlens, int n_seq, int max_len, int heads,
                           float scale, void* out_c_bf16, int ldo, float* lse_c, hipStream_t stream);
/* Its backward: from dout_c(bf16) [n_seq, H*64], out_c and lse_c it writes the WHOLE dqkv(bf16) [T, 3*H*64] range of the call's
 * sequences -- dK and dV of every token, dQ of the cls row, exact ZEROS in every other dQ row (the dense qkv input-gradient GEMM and
 * weight gradient read them) -- and no row outside them.  P is recomputed in fp32 from lse_c, delta = sum(dO * O) from the stored
 * bf16 O; the sums are fp32; P and dS (formed from the unrounded P) are rounded to bf16 in registers where lafs_attention_bwd
 * rounds them (in front of the products that give dV and dK / dQ), and 16 bits are STORED exactly once per value of dqkv. */
int lafs_attention_cls_bwd(const void* qkv, int ldqkv, const void* out_c_bf16, int ldo, const void* dout_c_bf16, int lddo,
                           const float* lse_c, const int32_t* cu_seqlens, int n_seq, int max_len, int heads, float scale,
                           void* dqkv, int lddqkv, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Patch embedding front end  (vision_transformer.py:126-131, 196-207; face_pre_pro/ViT_face.py:760-766)
 * ------------------------------------------------------------------------------------------------ */
enum { LAFS_PATCH_ORDER_CHW = 0 /* Conv2d weight [D,c,p1,p2] */, LAFS_PATCH_ORDER_HWC = 1 /* '(p1 p2 c)' */ };
/* img(f32) [B,3,S,S] -> patches(bf16) [B*(S/p)^2, 3*p*p], p = 8. */
int lafs_patchify(const float* img, int B, int S, int order, void* patches, hipStream_t stream);
/* tokens(f32)[b*(np+1), :] = cls[:] + pos[0,:]  for every sequence (the patch rows are written by the
 * LAFS_EPI_EMBED_F32 GEMM epilogue). */
int lafs_embed_cls(const float* cls, const float* pos, float* tokens, int ldt, int n_seq, int npatch, int D,
                   hipStream_t stream);
/* Backward of the token assembly: g(f32) [n_seq*(np+1), D] ->
 *   gp(bf16) [n_seq*np, D] (patch rows only), dpos(f32)[np+1, D] += sum over sequences, dcls(f32)[D] += sum g[cls rows].
 * workspace (f32, lafs_embed_bwd_workspace_bytes; may be NULL): with it every chunk of 16 sequences stores its sums into a slot of its
 * own and a second launch adds the slots in ascending order -- run-to-run deterministic gradients of the position table and the cls
 * token; without it the sums leave as one fp32 atomic per element and chunk (round 1-5 behaviour). */
int64_t lafs_embed_bwd_workspace_bytes(int n_seq, int npatch, int D);
int lafs_embed_bwd(const float* g, int ldg, int n_seq, int npatch, int D, void* gp, float* dpos, float* dcls,
                   float* workspace, hipStream_t stream);
/* feat(bf16 and/or f32) [n_seq, D] = x[row of cls token of each sequence]; and its scatter-back. */
int lafs_gather_cls(const float* x, int ldx, const int32_t* cu_seqlens, int n_seq, int D, float* out_f32,
                    hipStream_t stream);
/* g(f32)[first row of each sequence, :] = src[n_seq, D]  (g is expected to be zero elsewhere). */
int lafs_scatter_cls(const float* src, const int32_t* cu_seqlens, int n_seq, int D, float* g, int ldg,
                     hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * fViT: overlapping patch embedding and BatchNorm1d head  (face_pre_pro/ViT_face.py:1506-1613; csrc/unfold.hip)
 * ------------------------------------------------------------------------------------------------ */
/* nn.Unfold(kernel_size=k, stride, padding=pad) + transpose(1, 2) (face_pre_pro/ViT_face.py:1517,1582):
 * img(f32) [B,3,S,S] -> patches(bf16) [B*n*n, ldp], n = floor((S + 2 pad - k) / stride) + 1 windows per side.  Column c k^2 + i k + j of
 * row (b, wy, wx) = img[b, c, wy stride - pad + i, wx stride - pad + j], 0 for a tap outside the image; columns [3 k^2, ldp) are 0
 * (ldp % 32 == 0: the K granule of lafs_gemm_nt).  Same bf16 rounding as lafs_patchify: (k, stride, pad) = (8, 8, 0), ldp = 192 gives
 * its LAFS_PATCH_ORDER_CHW rows bit for bit.  The image needs no alignment; patches must be 16-byte aligned.  k >= 1, stride >= 1,
 * 0 <= pad < k, n >= 1; one window row of the three channels (3 k ((n-1) stride + k) floats) must fit 64 KB of LDS. */
int lafs_unfold_bf16(const float* img, int B, int S, int k, int stride, int pad, void* patches, int ldp, hipStream_t stream);
/* The adjoint (autograd of :1582 when the image requires a gradient): dpatches(f32) [B*n*n, ld] (columns >= 3 k^2 ignored) ->
 * dimg(f32) [B,3,S,S], WRITTEN: every pixel is the sum of the window entries that cover it, window rows then window columns ascending
 * (no atomics, the same bits run to run); a pixel under no window is 0. */
int lafs_fold_f32(const float* dpatches, int ld, int B, int S, int k, int stride, int pad, float* dimg, hipStream_t stream);
/* dst(bf16)[r, c] = src(f32)[r, c] for c < cols, 0 for cols <= c < ldd (ldd % 8 == 0, dst 16-byte aligned): the Linear weight
 * [D, 3 k^2] of :1521,1585 and ready-made 3-D patch vectors (:1583-1584) widened to the ldp columns of lafs_unfold_bf16. */
int lafs_pad_cast_bf16(const float* src, int lds, int rows, int cols, void* dst, int ldd, hipStream_t stream);
/* dst(f32)[r, c] = (accumulate ? dst[r, c] : 0) + src[r, c] for c < cols: the first 3 k^2 columns of the ldp-wide weight gradient
 * into the [D, 3 k^2] gradient of :1521. */
int lafs_add_cols_f32(const float* src, int lds, int rows, int cols, float* dst, int ldd, int accumulate, hipStream_t stream);
/* nn.BatchNorm1d(D) on x f32 [n, D] (the mlp_head of :1530-1533,1604).  training != 0 (n >= 2): per column mean and biased variance
 * (shifted two-pass sums, fixed order, no atomics), y = (x - mean) rstd gamma + beta with rstd = 1 / sqrt(var + eps); running_mean /
 * running_var (both or neither) become (1 - momentum) old + momentum {mean, var n / (n - 1)}.  training == 0: mean = running_mean,
 * rstd = 1 / sqrt(running_var + eps), nothing updated.  save_mean / save_rstd f32 [D] receive what y was formed with. */
int lafs_bn1d_fwd(const float* x, int ldx, int n, int D, const float* gamma, const float* beta, float eps, float momentum,
                  int training, float* running_mean, float* running_var, float* y, int ldy, float* save_mean, float* save_rstd,
                  hipStream_t stream);
/* Backward: xhat = (x - save_mean) save_rstd; dgamma = (accumulate ? dgamma : 0) + sum_r dy xhat, dbeta likewise + sum_r dy;
 * dx = gamma rstd (dy - dbeta_batch / n - xhat dgamma_batch / n) in training, gamma rstd dy in eval (constant statistics). */
int lafs_bn1d_bwd(const float* dy, int lddy, const float* x, int ldx, int n, int D, const float* save_mean, const float* save_rstd,
                  const float* gamma, int training, float* dx, int lddx, float* dgamma, float* dbeta, int accumulate,
                  hipStream_t stream);
/* The same head over G crop groups of one packed pass (face_pre_pro/ViT_face.py:1530-1533,1556-1569: forward() runs the head once per
 * run of equal-sided crops, in list order), one launch: group g is the rows [group_rows[g], group_rows[g + 1]) of x / y / dy / dx.
 * group_rows is a HOST array of G + 1 ascending row numbers, group_rows[0] = 0, 1 <= G <= LAFS_BN1D_MAX_GROUPS; it is copied into the
 * launch by value, so nothing is read from it after the call returns and the launch can be captured.  The result is bit for bit that
 * of G lafs_bn1d_fwd / lafs_bn1d_bwd calls on the row ranges in group order (the same arithmetic, no atomics): every group has its own
 * mean, biased variance and rstd (save_mean / save_rstd f32 [G, D], row g for group g); in training the running buffers take the
 * (1 - momentum) old + momentum new update once per group, group 0 first, the unbiased variance with that group's own row count, and
 * every group needs >= 2 rows; training == 0: every group is normalised with the running statistics, nothing is updated.
 * Backward: dgamma / dbeta = (accumulate ? old : 0) + the groups' sums added in group order; dx per group as lafs_bn1d_bwd. */
#define LAFS_BN1D_MAX_GROUPS 8
int lafs_bn1d_groups_fwd(const float* x, int ldx, const int* group_rows, int G, int D, const float* gamma, const float* beta, float eps,
                         float momentum, int training, float* running_mean, float* running_var, float* y, int ldy, float* save_mean,
                         float* save_rstd, hipStream_t stream);
int lafs_bn1d_groups_bwd(const float* dy, int lddy, const float* x, int ldx, const int* group_rows, int G, int D, const float* save_mean,
                         const float* save_rstd, const float* gamma, int training, float* dx, int lddx, float* dgamma, float* dbeta,
                         int accumulate, hipStream_t stream);
/* The grouped head in training mode with the statistics of ALL ranks: what nn.SyncBatchNorm.convert_sync_batchnorm (reference
 * lafs_train.py:362-364) makes of the BatchNorm1d of face_pre_pro/ViT_face.py:1530-1533 in the per-group forward of :1556-1569.
 * Forward and backward are each cut where the ranks meet; the exchange between the two halves is the caller's (torch.distributed,
 * outside the graphs).  group_rows is this rank's row table as above, except that a group may hold a SINGLE row on a rank (no empty
 * group); group_total is a HOST table of the G total row counts over all ranks (by value, like group_rows; each >= 2, >= this rank's
 * own count, <= 2^24).  All four launches can be captured, use no atomics and walk the groups in order, one workgroup per 64 columns.
 *
 * lafs_bn1d_groups_stats: this rank's partial statistics, partial f32 [G, 1 + 2 D] = per group {count, mean[D], M2[D]}, mean the
 *   shifted sum and M2 = sum (x - mean)^2 the second pass of lafs_bn1d_fwd, operation for operation (one row: M2 = 0).
 * lafs_bn1d_groups_sync_fwd: partials f32 = the W ranks' partials, rank r at partials + r ldw (ldw >= G (1 + 2 D) floats; W <=
 *   LAFS_BN1D_MAX_RANKS).  Per group and column they are folded in rank order 0 .. W-1 with
 *     n = n_a + n_b, delta = mean_b - mean_a, mean = mean_a + delta n_b / n, M2 = M2_a + M2_b + delta^2 n_a n_b / n
 *   (the counts come from the partials), rstd = 1 / sqrt(M2 / N + eps); save_mean / save_rstd f32 [G, D]; the running buffers (both
 *   or neither) take (1 - momentum) old + momentum {mean, M2 / N * (N / (N - 1))} once per group, group 0 first; y = this rank's rows
 *   normalised.  The order is fixed, so every rank that is given the same partials computes the same bits.  W = 1: every output has
 *   the bits of lafs_bn1d_groups_fwd (training).
 * lafs_bn1d_groups_bwd_sums: sums f32 [G, 2 D] = per group {sum_r dy [D], sum_r dy xhat [D]} over this rank's rows, and dgamma /
 *   dbeta = (accumulate ? old : 0) + those sums added in group order: rank-local, as in torch's SyncBatchNorm (the gradient
 *   all-reduce treats them like every other parameter gradient).
 * lafs_bn1d_groups_sync_bwd: sums = the sums of all ranks added up; dx = gamma rstd (dy - sum dy / N - xhat sum(dy xhat) / N) for this
 *   rank's rows, N = group_total[g].  With the sums of the one rank (W = 1) the two launches give the bits of lafs_bn1d_groups_bwd. */
#define LAFS_BN1D_MAX_RANKS 4096
int lafs_bn1d_groups_stats(const float* x, int ldx, const int* group_rows, int G, int D, float* partial, hipStream_t stream);
int lafs_bn1d_groups_sync_fwd(const float* x, int ldx, const int* group_rows, const int* group_total, int G, int D, const float* partials,
                              int W, int64_t ldw, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                              float* running_var, float* y, int ldy, float* save_mean, float* save_rstd, hipStream_t stream);
int lafs_bn1d_groups_bwd_sums(const float* dy, int lddy, const float* x, int ldx, const int* group_rows, int G, int D,
                              const float* save_mean, const float* save_rstd, float* sums, float* dgamma, float* dbeta, int accumulate,
                              hipStream_t stream);
int lafs_bn1d_groups_sync_bwd(const float* dy, int lddy, const float* x, int ldx, const int* group_rows, const int* group_total, int G,
                              int D, const float* save_mean, const float* save_rstd, const float* gamma, const float* sums, float* dx,
                              int lddx, hipStream_t stream);
/* DINOHead(use_bn=True): nn.BatchNorm1d(hidden_dim) + nn.GELU() behind a hidden Linear (vision_transformer.py:272-281: :274-275 and
 * :279-280), fused.  u f32 [n, D] (row stride ldu) is the Linear's output; a bf16 [n, D] (row stride lda) = gelu(xhat gamma + beta),
 * the erf GELU of the GEMM epilogues; the BatchNorm output itself is never stored.  Statistics, rstd = 1 / sqrt(var + eps), the
 * running-buffer update (both or neither; unbiased variance), training == 0 and save_mean / save_rstd f32 [D] are exactly those of
 * lafs_bn1d_fwd (the same device functions: same bits); training needs n >= 2, checked before any launch.  Columns >= D and rows >= n
 * are neither read nor written; D needs no alignment.  No atomics: two runs give the same bits. */
int lafs_bn1d_gelu_fwd(const float* u, int ldu, int n, int D, const float* gamma, const float* beta, float eps, float momentum,
                       int training, float* running_mean, float* running_var, void* a_bf16, int lda, float* save_mean,
                       float* save_rstd, hipStream_t stream);
/* Backward: xhat = (u - save_mean) save_rstd and y = xhat gamma + beta are recomputed, g = da gelu'(y) (da f32 [n, D], the gradient of
 * a); dbeta = (accumulate ? dbeta : 0) + sum_r g, dgamma likewise + sum_r g xhat; du bf16 [n, D] = gamma rstd (g - sum g / n -
 * xhat sum(g xhat) / n) in training, gamma rstd g in eval.  One launch, two passes over the rows; g is never stored. */
int lafs_bn1d_gelu_bwd(const float* da, int ldda, const float* u, int ldu, int n, int D, const float* save_mean, const float* save_rstd,
                       const float* gamma, const float* beta, int training, void* du_bf16, int lddu, float* dgamma, float* dbeta,
                       int accumulate, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DINO head pieces  (vision_transformer.py:284-287, 299-300)
 * ------------------------------------------------------------------------------------------------ */
/* y = x / max(||x||_2, 1e-12) row-wise: x f32 [rows, D] -> y bf16 (+ inv_norm f32 [rows]). */
int lafs_l2norm_fwd(const float* x, int ldx, void* y_bf16, int ldy, float* inv_norm, int rows, int D,
                    hipStream_t stream);
/* dx(f32) = inv_norm * (dy - y * <y, dy>)   with y recomputed from x. */
int lafs_l2norm_bwd(const float* x, int ldx, const float* dy, int lddy, const float* inv_norm, float* dx, int lddx,
                    int rows, int D, hipStream_t stream);
/* weight_norm (dim=0): w(bf16)[k,:] = g[k] * v[k,:] / ||v[k,:]|| ; also w_t(bf16) [D, ldwt] transposed copy
 * (NULL to skip); rows k in [K, Kpad) of w and columns of w_t are zero-filled.  inv_norm f32 [K].  An all-zero row of v gives
 * inv_norm = inf and a NaN row of w, as in torch: there is no clamp. */
int lafs_weightnorm_fwd(const float* v, const float* g, int K, int Kpad, int D, void* w, void* w_t, int ldwt,
                        float* inv_norm, hipStream_t stream);
/* dv(f32)[k,:] (+)= g/||v|| * (dw - vhat * <dw, vhat>) ; dg(f32)[k] (+)= <dw, vhat>  (dg may be NULL). */
int lafs_weightnorm_bwd(const float* dw, const float* v, const float* g, const float* inv_norm, int K, int D,
                        float* dv, float* dg, int accumulate, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DINO loss (lafs_train.py:643-679), closed form:
 *   q_i = softmax((t_i - c)/tau_t),  p_v = softmax(s_v / tau_s)
 *   loss = 1/n_terms * sum_{i in {0,1}, v != i} mean_b [ lse(s_v/tau_s) - <q_i, s_v/tau_s> ]
 *   dL/ds_v = 1/(n_terms * B * tau_s) * sum_{i != v} (p_v - q_i)
 * student f32 [ncrops*B, ld], teacher f32 [2*B, ld], center f32 [K]; grad bf16 or f32 [ncrops*B, ldg].
 * workspace f32: lafs_dino_loss_workspace(ncrops, B, K) floats.  dev_temps (optional, device f32[2] =
 * {student_temp, teacher_temp}) overrides the two host values so that a captured hipGraph follows the
 * teacher-temperature schedule.
 * ------------------------------------------------------------------------------------------------ */
int64_t lafs_dino_loss_workspace(int ncrops, int B, int K);
int lafs_dino_loss_fwd_bwd(const float* student, const float* teacher, int ld, const float* center, int ncrops,
                           int B, int K, float student_temp, float teacher_temp, float* loss_out,
                           void* grad, int ldg, int grad_is_bf16, float grad_scale, float* workspace,
                           const float* dev_temps, hipStream_t stream);
/* DINOHead's last layer of BOTH networks + DINOLoss.forward + the row sums of update_center in one piece (vision_transformer.py:
 * 295-301, lafs_train.py:643-679): the [ncrops B + 2 B, K] logits are formed twice on the MFMA (a K = 256 contraction per class) and
 * never stored.  zn_*: bf16 [rows, 256] L2-normalised bottleneck rows (student: ncrops B rows in crop-major order, teacher: 2 B),
 * wn_*: bf16 [Kpad, 256] weight-normalised last-layer rows (pad rows zero), center f32 [K].  Outputs: loss_out f32 [1];
 * grad_bf16 [ncrops B, ldg] = grad_scale * dL/d(student logits) (pad columns K..Kpad zero); colsum_out f32 [K] (optional) =
 * sum over the teacher rows of the raw teacher logits.  Same closed form as lafs_dino_loss_fwd_bwd; no atomics: deterministic.
 * dim must be 256, B <= 64, Kpad % 8 == 0.  workspace f32: lafs_dino_head_loss_workspace(ncrops, B, K) floats. */
int64_t lafs_dino_head_loss_workspace(int ncrops, int B, int K);
int lafs_dino_head_loss(const void* zn_student, const void* zn_teacher, const void* wn_student, const void* wn_teacher, int dim,
                        const float* center, int ncrops, int B, int K, int Kpad, float student_temp, float teacher_temp,
                        const float* dev_temps, float* loss_out, void* grad_bf16, int ldg, float grad_scale, float* colsum_out,
                        float* workspace, hipStream_t stream);
/* colsum(f32)[k] = sum_rows teacher[r, k]   (lafs_train.py:674; all-reduced by the caller) */
int lafs_colsum_f32(const float* x, int ld, int rows, int K, float* out, hipStream_t stream);
/* center = center*m + colsum/(rows_total) * (1-m)   (lafs_train.py:676-679) */
int lafs_center_ema(float* center, const float* colsum, int K, float inv_rows_total, float momentum,
                    hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-tensor step glue over a flat parameter arena split into 1024-element chunks
 *   utils.py:132-141 (per-tensor clip), lafs_train.py:400 + torch AdamW, lafs_train.py:610-613 (EMA)
 * chunk_seg(i32)[n_chunks] maps each chunk to its tensor (segment).  seg_flags bit0 = weight decay on,
 * bit1 = "last_layer" (skipped while frozen), bit2 = trainable.  Hyper-parameters live in a device f32[16]:
 * {lr, wd, beta1, beta2, eps, clip, ema_m, freeze_last_layer(0/1), grad_scale, ...}.
 * ------------------------------------------------------------------------------------------------ */
#define LAFS_N_XCD 8          /* XCDs (L2 domains) of an MI355X */
#define LAFS_CHUNK 1024
enum { LAFS_SEG_DECAY = 1, LAFS_SEG_LAST_LAYER = 2, LAFS_SEG_TRAINABLE = 4,
       LAFS_SEG_OVERWRITTEN = 16 /* the step's first gradient writer of this tensor OVERWRITES it (wgrad fold with accumulate = 0,
                                     weight-norm backward): lafs_zero_chunks(skip_mask = 16) leaves it alone */,
       LAFS_SEG_LOW_DECAY = 8 /* decays at hyper[LAFS_HP_WD_LOW] instead of hyper[LAFS_HP_WD]: the `stn*` matrices of the
                                  fine-tune step, train_largescale.py:143-145 (5e-2 against 1e-1) */ };
enum { LAFS_HP_LR = 0, LAFS_HP_WD, LAFS_HP_BETA1, LAFS_HP_BETA2, LAFS_HP_EPS, LAFS_HP_CLIP, LAFS_HP_EMA_M,
       LAFS_HP_FREEZE_LAST, LAFS_HP_GRAD_SCALE, LAFS_HP_WD_LOW,
       LAFS_HP_STEP /* optimisation step count (as a float): seeds the per-step DropPath masks of a replayed graph */,
       LAFS_HP_MIX_LAM /* mixup lambda of this fine-tune micro-step (lam_dev of lafs_mixup_normalize / lafs_margin_softmax_ce_bf16) */,
       LAFS_HP_LAND_W /* weight of the landmark-supervision term of this fine-tune micro-step (`weight` of lafs_landmark_mse) */,
       LAFS_HP_MOMENTUM = 13 /* momentum of the SGD / LARS buffer: 0.9, torch.optim.SGD(..., momentum=0.9) at lafs_train.py:402 and the
                                default of utils.LARS (utils.py:557) */,
       LAFS_HP_LARS_ETA = 14 /* LARS trust coefficient eta: 0.001, the default of utils.LARS (utils.py:557) */,
       LAFS_HP_COUNT = 16 };
/* seg_sumsq(f32)[n_seg] = sum of (grad_scale*g)^2 per segment -- the per-tensor norms of utils.clip_gradients
 * (utils.py:132-141).  Two passes through chunk_sumsq(f32)[n_chunks] scratch, fixed summation order: no atomics, nothing
 * to pre-zero, bitwise reproducible. */
int lafs_grad_sumsq(const float* grad, const int32_t* chunk_seg, int64_t n_chunks, int n_seg, const float* hyper,
                    float* chunk_sumsq, float* seg_sumsq, hipStream_t stream);
/* Fused per-tensor clip + AdamW + teacher EMA + bf16 shadow refresh.  seg_step(i32)[n_seg] counts the
 * optimizer steps each tensor has actually taken.  teacher/shadow pointers may be NULL. */
int lafs_clip_adamw_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* teacher,
                        void* param_bf16, void* teacher_bf16, const int32_t* chunk_seg, int64_t n_chunks,
                        const int32_t* seg_flags, int32_t* seg_step, int n_seg, const float* seg_sumsq,
                        const float* hyper, hipStream_t stream);
/* The same two passes restricted to the tensors [seg_lo, seg_hi) = the chunks [chunk_lo, chunk_hi) (base pointers are those of the
 * whole arena): the engine updates a range of the arena as soon as its gradients are final, beside the rest of the backward. */
int lafs_grad_sumsq_range(const float* grad, const int32_t* chunk_seg, int64_t n_chunks, int n_seg, int64_t chunk_lo, int64_t chunk_hi,
                          int seg_lo, int seg_hi, const float* hyper, float* chunk_sumsq, float* seg_sumsq, hipStream_t stream);
/* n_chunks / n_seg are the sizes of the WHOLE arena: a range that leaves them is refused (LAFS_ESHAPE), not clipped. */
int lafs_clip_adamw_ema_range(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* teacher,
                              void* param_bf16, void* teacher_bf16, const int32_t* chunk_seg, int64_t n_chunks, int64_t chunk_lo,
                              int64_t chunk_hi, const int32_t* seg_flags, int32_t* seg_step, int n_seg, int seg_lo, int seg_hi,
                              const float* seg_sumsq, const float* hyper, hipStream_t stream);
/* The update rules behind --optimizer sgd / lars (lafs_train.py:401-404).  Both keep ONE state buffer, `mom` (torch's momentum_buffer,
 * LARS's mu), and couple the decay into the gradient: with g^ the scaled and clipped gradient of lafs_clip_adamw_ema,
 *   SGD  (torch.optim.SGD, momentum = hyper[LAFS_HP_MOMENTUM], dampening 0, no Nesterov; lafs_train.py:402)
 *        d = g^ + wd_t p        wd_t: hyper[LAFS_HP_WD] / hyper[LAFS_HP_WD_LOW] / 0 by the tensor's LAFS_SEG_DECAY / LAFS_SEG_LOW_DECAY bits
 *   LARS (utils.py:553-591)  LAFS_SEG_DECAY set (ndim != 1, utils.py:573-583):  d = q (g^ + wd_t p),
 *        q = eta ||p|| / ||g^ + wd_t p|| where both norms are > 0, else 1;  LAFS_SEG_DECAY clear (ndim == 1):  d = g^
 *   both (utils.py:585-591):  mom = momentum * mom + d;  p -= lr * mom
 * A zero `mom` gives the first step's buf = d of torch, so neither rule reads seg_step -- which still counts the steps a tensor
 * has taken (checkpoints, the DropPath seed). */
enum { LAFS_UPDATE_SGD = 1, LAFS_UPDATE_LARS = 2 };
/* lafs_grad_sumsq_range for a LARS step: seg_sumsq exactly as there (same order, same bits), and seg_trust(f32)[n_seg] = q of the
 * tensors [seg_lo, seg_hi) (1 where LAFS_SEG_DECAY is clear), from ONE read of grad and param: per chunk sum g^2, sum p^2, sum g p
 * into chunk_part(f32)[3 * n_chunks] (three planes of n_chunks), per tensor
 *   ||g^ + wd p||^2 = gsc^2 sum g^2 + 2 gsc wd sum g p + wd^2 sum p^2,   gsc = grad_scale * min(1, clip coefficient)
 * replacing torch.norm(p), torch.norm(dp) of utils.py:577-578.  No atomics, nothing to pre-zero, fixed summation order. */
int lafs_grad_sumsq_trust_range(const float* param, const float* grad, const int32_t* chunk_seg, int64_t n_chunks, int n_seg,
                                int64_t chunk_lo, int64_t chunk_hi, int seg_lo, int seg_hi, const int32_t* seg_flags, const float* hyper,
                                float* chunk_part, float* seg_sumsq, float* seg_trust, hipStream_t stream);
/* Fused per-tensor clip + SGD-with-momentum or LARS (kind: LAFS_UPDATE_*) + teacher EMA + bf16 shadow refresh on the tensors
 * [seg_lo, seg_hi): optimizer.step() of lafs_train.py:598,606 for the optimizers of :402 / :404 with the clip, freeze, EMA and shadow
 * handling of lafs_clip_adamw_ema_range.  seg_trust: what lafs_grad_sumsq_trust_range wrote (LARS; NULL for SGD).  teacher / shadow
 * pointers may be NULL.  An unknown kind, LARS without seg_trust, or a range that leaves the arena is refused (LAFS_ESHAPE). */
int lafs_clip_momentum_ema_range(int kind, float* param, const float* grad, float* mom, float* teacher, void* param_bf16,
                                 void* teacher_bf16, const int32_t* chunk_seg, int64_t n_chunks, int64_t chunk_lo, int64_t chunk_hi,
                                 const int32_t* seg_flags, int32_t* seg_step, int n_seg, int seg_lo, int seg_hi, const float* seg_sumsq,
                                 const float* seg_trust, const float* hyper, hipStream_t stream);
/* dst(bf16)[i] = src(f32)[i] */
int lafs_cast_bf16(const float* src, void* dst, int64_t n, hipStream_t stream);
/* dst(f32)[i] = src(bf16)[i]   (gradients that travelled over the wire as bf16: LAFS_GRAD_WIRE=bf16, distributed.py) */
int lafs_cast_f32(const void* src, float* dst, int64_t n, hipStream_t stream);
/* dst(bf16)[c, r] = src(bf16)[r, c]: operand transposes of the fine-tune margin head (dL/dcos [B, C] -> [C, B] feeds both class-
 * gradient GEMMs, train_largescale.py:820-867's autograd through ViT_face.py:49-89; was a torch .t().contiguous()). */
int lafs_transpose_bf16(const void* src, int rows, int cols, int ld_src, void* dst, int ld_dst, hipStream_t stream);
/* dst(bf16)[c, r] = src(f32)[r, c]   (W^T shadows used by the dgrad GEMMs) */
int lafs_transpose_cast_bf16(const float* src, int rows, int cols, void* dst, int ld_dst, hipStream_t stream);
/* All W^T shadows of an arena in ONE launch.  table(i64, device)[4*i..] = {src offset into master, rows, cols, dst offset
 * into shadow_t}; tile_start(i32, device)[n_mat+1] = prefix sum of each matrix's 64x64-tile count; n_tiles = tile_start[n_mat]. */
int lafs_transpose_cast_table(const float* master, void* shadow_t, const int64_t* table, const int32_t* tile_start,
                              int n_mat, int n_tiles, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Transformer engine: whole pre-LN ViT trunk forward/backward over a packed token batch
 *   vision_transformer.py:107-113, 209-215; face_pre_pro/ViT_face.py:106-120, 184-213
 * Offsets are in ELEMENTS into the caller's arenas: `master` (f32 parameters), `shadow` (bf16 copy, same
 * offsets), `shadow_t` (bf16 transposed weights, offsets *_t), `grad` (f32, same offsets as master).
 * ------------------------------------------------------------------------------------------------ */
typedef struct lafs_block_offsets {
  int64_t ln1_g, ln1_b, w_qkv, b_qkv /* -1 if none */, w_proj, b_proj, ln2_g, ln2_b, w_fc1, b_fc1, w_fc2, b_fc2;
  int64_t w_qkv_t, w_proj_t, w_fc1_t, w_fc2_t;     /* into shadow_t */
} lafs_block_offsets;

typedef struct lafs_trunk_desc {
  int dim, inner /* heads*64 */, heads, mlp, depth;
  float ln_eps, attn_scale;
  int n_tok, n_seq, max_len;
  const int32_t* cu_seqlens;      /* device i32 [n_seq+1] */
  const int32_t* row2seq;         /* device i32 [n_tok]   */
  const float* drop_scales;       /* device f32 [depth, 2, n_seq] or NULL */
  float dropout_p;                /* element dropout after to_out / after GELU / after fc2 (Part-fViT); 0 = off.  Site s of
                                     layer l uses seed dropout_seed + 3*l + s (s: 0 to_out, 1 GELU, 2 fc2)                 */
  uint32_t dropout_seed;
  const float* master; const void* shadow; const void* shadow_t; float* grad;
  const lafs_block_offsets* blocks;   /* HOST array [depth] */
  /* Sequence groups of equal length (the crop resolutions of a packed multi-crop batch, in packing order): attention is
   * launched once per group with the tile configuration of THAT length (197-token global crops: one (sequence, head) pair
   * per workgroup, 53 KB of LDS; 37-token local crops: four pairs per workgroup) instead of once with the longest one.
   * n_groups = 0: a single launch over all sequences with max_len. */
  int n_groups; int group_n_seq[4]; int group_max_len[4];
  int wgrad_workgroups;               /* CUs the grouped weight-gradient launch may occupy (0 = all 256), see lafs_wgrad_group */
  const float* dropout_step;          /* NULL or DEVICE pointer to the step counter added (x 7919) to dropout_seed inside the kernels */
  int wgrad_overwrite;                /* != 0: the block weight gradients are WRITTEN (not accumulated): the caller zeroes only the
                                         other tensors (lafs_zero_chunks, LAFS_SEG_OVERWRITTEN) and runs one backward per step */
  int wgrad_defer;                    /* != 0: lafs_trunk_backward launches NO weight-gradient GEMMs and keeps every layer's operands
                                         (dY of fc2 / fc1 / proj / qkv) in slots of their own -- the workspace grows by depth - 2 sets --
                                         until lafs_trunk_wgrad launches them, e.g. beside work that leaves the chip idle (the
                                         fine-tune step's landmark-CNN backward, train_largescale.py:785-891) */
  lafs_ctx* ctx;                      /* side streams / events / options of these passes (NULL: caller's stream only, default options) */
  int cls_only_last;                  /* != 0 (opt-in; 0 = every block dense, as before): the caller reads x_out only through the FIRST row of
                                         every sequence (the cls token) and hands lafs_trunk_backward a gradient that is zero in every other
                                         row.  The last block then runs LayerNorm 1 and the qkv GEMM on all rows (K and V are needed of every
                                         token) and everything behind them -- attention output, projection, LayerNorm 2, MLP -- on the n_seq cls
                                         rows only, forward and backward; its fc2 / fc1 / proj weight gradients sum over n_seq rows.  Of x_out
                                         ONLY the first row of every sequence is then defined.  Honoured where the plan allows
                                         (lafs_trunk_plan_info::cls_only_last).  The row-local compact activations live in the first n_seq rows of
                                         the block's own buffers (layer 0's set in a forward-only pass; written after the row chains have
                                         joined); the workspace grows by an n_seq identity table (written by the forward, read by the
                                         backward), two f32 [n_seq, dim] row sets and the cls attention's o_c [n_seq, inner] (bf16) /
                                         lse_c [n_seq, heads] -- the row chains write these while other chains may still run earlier blocks
                                         on the shared buffer set, so they alias nothing -- and, when saving, by what the n_seq-row
                                         weight-gradient launch's slice partials need beyond the dense launch's */
} lafs_trunk_desc;

/* Bytes of activation workspace for a forward with (1) / without (0) saving activations for backward.  The LayerNorm backward's
 * gamma / beta slot buffers are sized for four row chains whatever LAFS_OPT_ROW_CHAINS says: the option may change on a live
 * context after the workspace was sized. */
int64_t lafs_trunk_workspace_bytes(const lafs_trunk_desc* d, int save_for_backward);
/* What the trunk passes of this descriptor launch (csrc/engine.hip: plan): the ONE decision lafs_trunk_forward (with this
 * save_for_backward), lafs_trunk_backward and its LayerNorm fold read.  Host logic only: no HIP call, so with ctx == NULL it runs
 * without a device.  LAFS_OK, or the descriptor's refusal (text in lafs_last_error()).  Tests assert the route they mean to cover.
 * Launch counts are not part of it: they follow from lafs_gemm_nt_plan and from lafs_mlp_fused's own unit sizes. */
enum { LAFS_ATTN_ONE_LAUNCH = 0,       /* one attention launch over all sequences with max_len (n_groups <= 1) */
       LAFS_ATTN_PER_GROUP = 1,        /* one launch per crop-resolution group, on the row range's stream */
       LAFS_ATTN_PER_GROUP_FORKED = 2  /* one range, side streams: the second and later groups' launches on the first side stream */ };
typedef struct lafs_trunk_range_plan {
  int row0, rows;                      /* token rows [row0, row0 + rows) */
  int group, seq0, n_seq;              /* (first) sequence group, first sequence, sequences */
  int stream;                          /* 0: the caller's; i: the context's side stream i - 1.  Also the range's LayerNorm slot */
  int fwd_fused;                       /* forward: the MLP is one lafs_mlp_fused launch (else two GEMMs), with ... */
  int fwd_ln2_inside;                  /* ... LayerNorm 2 inside (not launched), */
  int fwd_next_ln1;                    /* ... the next block's LayerNorm 1 written by it: LayerNorm 1 of blocks 1.. is not launched, */
  int fwd_proj_inside;                 /* ... the attention projection + residual in front (their GEMM is not launched) */
  int bwd_fused;                       /* backward: the MLP input gradients are one launch (else two GEMMs), with ... */
  int bwd_ln2_inside;                  /* ... LayerNorm 2's backward inside (its gamma / beta slots fit the workspace's) */
  int ln1_parts, ln2_parts;            /* gamma / beta partial slots the backward of each norm writes (lafs_layernorm_bwd_fold adds them) */
} lafs_trunk_range_plan;
typedef struct lafs_trunk_plan_info {
  int n_ranges;                        /* independent chains of launches: 2 (4: half groups) with side streams, LAFS_OPT_ROW_CHAINS >= 2 (4)
                                          and two crop-resolution groups of >= 4096 full-length rows each, else 1 */
  int attention;                       /* LAFS_ATTN_* */
  int mlp_merged;                      /* forward: the ranges meet in front of every MLP, which is ONE launch over `whole` */
  lafs_trunk_range_plan range[4];      /* [n_ranges]; with mlp_merged their fwd_* describe the merged launch */
  lafs_trunk_range_plan whole;         /* all rows as one range (= range[0] when n_ranges == 1) */
  int cls_only_last;                   /* the last block runs on the cls rows behind its qkv GEMM: lafs_trunk_desc::cls_only_last is set, and
                                          dropout_p == 0 (element-dropout masks are indexed by absolute row: a compacted row loses it), and
                                          wgrad_defer == 0 (the deferred weight gradients read dense operand slots), and the pass includes
                                          block depth - 1 (every forward; a backward with layer_hi == depth).  Its LayerNorm-2 backward then
                                          writes lafs_layernorm_bwd_parts(n_seq, dim) gamma / beta slots into chain 0's buffer and none elsewhere */
} lafs_trunk_plan_info;
int lafs_trunk_plan(const lafs_trunk_desc* d, int save_for_backward, lafs_trunk_plan_info* out);
/* The plan of a pass over blocks layer_hi-1 .. layer_lo only (lafs_trunk_backward walks the trunk in such slices); lafs_trunk_plan is
 * the whole trunk, (depth, 0).  The range decides cls_only_last, nothing else. */
int lafs_trunk_plan_layers(const lafs_trunk_desc* d, int save_for_backward, int layer_hi, int layer_lo, lafs_trunk_plan_info* out);
/* The plan's n_ranges; -1 for a refused descriptor. */
int lafs_trunk_row_ranges(const lafs_trunk_desc* d);
/* x_in(f32) [n_tok, dim] -> x_out(f32) [n_tok, dim]: residual stream after the last block.  With
 * save_for_backward != 0 x_in must stay untouched until lafs_trunk_backward has run (it is layer 0's saved input)
 * and must not alias x_out.  With the plan's cls_only_last only the first row of every sequence of x_out is defined (the other rows
 * keep whatever the buffer held or received as a ping-pong buffer of the earlier blocks). */
int lafs_trunk_forward(const lafs_trunk_desc* d, const float* x_in, float* x_out, void* workspace,
                       int save_for_backward, hipStream_t stream);
/* g(f32) [n_tok, dim]: dL/dx_out on entry, dL/dx_in on exit.  Parameter gradients are ACCUMULATED into d->grad.
 * Blocks layer_hi-1 .. layer_lo run; pass (depth, 0) for the whole trunk, or walk it in slices to start the
 * gradient all-reduce of finished blocks early.  wgrad_stream (optional, may be NULL or == stream): the weight-gradient
 * GEMMs are enqueued there and overlap the dgrad / attention / LayerNorm chain on `stream` (forked and joined with
 * events, so the call is still hipGraph-capturable and complete on `stream` when it returns to stream order).
 * With the plan's cls_only_last (layer_hi == depth) g must be zero on entry outside the first row of every sequence: the last block's
 * residual branches take their upstream gradient from those rows alone. */
int lafs_trunk_backward(const lafs_trunk_desc* d, const float* x_in, float* g, void* workspace, int layer_hi,
                        int layer_lo, hipStream_t wgrad_stream, hipStream_t stream);
/* The weight gradients (and bias gradients) of blocks layer_hi-1 .. layer_lo that a lafs_trunk_backward with d->wgrad_defer set
 * left out: one grouped launch per block on `stream` (at most d->wgrad_workgroups workgroups each), reading the per-layer operand
 * slots of `workspace`.  Same kernels, same operands, same accumulate / overwrite rule as the immediate form: identical results.
 * Replaces autograd's dW = dY^T X of the block linears (vision_transformer.py:59-65, 75-90; face_pre_pro/ViT_face.py:126-149). */
int lafs_trunk_wgrad(const lafs_trunk_desc* d, void* workspace, int layer_hi, int layer_lo, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Step glue that used to run on ATen / rocBLAS inside the captured step (csrc/stepglue.hip)
 * ------------------------------------------------------------------------------------------------ */
/* Stochastic depth (vision_transformer.py:27-35; ViT_face.py:106-112): scales(f32)[depth, 2, n_seq] = 1/keep_l with probability
 * keep_l, else 0; keep_prob f32 [depth] on the device.  Counter-based: hash(seed, step, index), `step_dev` (device f32, may be
 * NULL) = &hyper[LAFS_HP_STEP], so a replayed hipGraph draws new masks every step.  Same distribution as torch.rand-based
 * drop_path, different random stream. */
int lafs_droppath_scales(const float* keep_prob, int depth, int n_seq, uint32_t seed, const float* step_dev, float* scales,
                         hipStream_t stream);
/* interpolate_pos_encoding (vision_transformer.py:174-194) as its fixed linear map: out(f32)[1+R, D]: row 0 = cls row of the
 * table, rows 1.. = interp(f32 [R, G]) @ table[1:, :]  (table f32 [1+G, D]).  bwd: grad_table += the transposed map of dpos. */
int lafs_pos_interp_fwd(const float* pos_table, const float* interp, float* out, int R, int G, int D, hipStream_t stream);
int lafs_pos_interp_bwd(const float* dpos, const float* interp, float* grad_table, int R, int G, int D, hipStream_t stream);
/* Zero the 1024-float chunks of a gradient arena whose segment flags do not intersect skip_mask. */
int lafs_zero_chunks(float* buf, const int32_t* chunk_seg, const int32_t* seg_flags, int64_t n_chunks, int skip_mask,
                     hipStream_t stream);
/* buf[0 .. bytes) = 0 as a kernel launch on `stream` (16-byte aligned buffer). */
int lafs_fill_zero(void* buf, int64_t bytes, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fine-tune path (train_largescale.py): margin-softmax head, mixup, landmark patch gather
 * ------------------------------------------------------------------------------------------------ */
/* CosFace logits + soft-target CE, fused over the class axis (face_pre_pro/ViT_face.py:49-89;
 * timm SoftTargetCrossEntropy, train_largescale.py:820).  cos(f32) [B, ld] holds x_hat . w_hat^T on entry and
 * dL/dcos on exit.  The (mixup) target is given sparsely: y1,y2 (i32 [B]) with weights lam,(1-lam).
 * loss_out(f32)[1] = mean_b CE.  margin_type 0 = CosFace s*(cos - m*y), 1 = ArcFace (hard labels only).
 * One workgroup per row, one launch (the row loss is formed before the row is overwritten).  The target, the log-sum-exp and the
 * gradient expression are the ones of the two chunked entry points below: one implementation, three shapes of launch. */
int lafs_margin_softmax_ce(float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2, float lam,
                           float s, float m, int margin_type, float loss_scale, float* loss_out, float* row_ws,
                           hipStream_t stream);
/* Class-sharded margin softmax (PartialFC; PARITY UNPINNED: absent from the reference, ViT_face.py:645-649 is a commented
 * import; semantics follow InsightFace partial_fc_v2).  cos(f32) [B, ld] over this rank's S (sampled) class centres;
 * y_local(i32)[B] = local index of the target or -1.  Soft (mixup) targets as the reference always feeds its margin head
 * (train_largescale.py:802; dense lam e_y1 + (1 - lam) e_y2 entering the margin itself, ViT_face.py:69-73): y2_local(i32)[B] = local
 * index of the mixup partner's class or -1, lam(f32)[B] = the row's lambda (NULL: 1); y2_local == NULL: hard labels.  CosFace only.
 * Three passes with the cross-rank statistics exchanged in between (all-reduce MAX of rowmax, all-reduce SUM of rowsum and
 * target_logit):  z = margin logits s (cos - m y);
 *   rowmax[b] = max_k z ;  rowsum[b] = sum_k exp(z - gmax[b]), target_logit[b] = sum over the targets this rank owns of y_k z_k ;
 *   grad (in place) cos <- grad_scale * (exp(z - gmax)/Z - y) * dz/dcos.      loss_b = log Z + gmax - target_logit. */
int lafs_shard_margin_rowmax(const float* cos, int ld, int B, int S, const int32_t* y_local, const int32_t* y2_local, const float* lam,
                             float s, float m, int margin_type, float* rowmax, hipStream_t stream);
int lafs_shard_margin_rowsum(const float* cos, int ld, int B, int S, const int32_t* y_local, const int32_t* y2_local, const float* lam,
                             float s, float m, int margin_type, const float* gmax, float* rowsum, float* target_logit, hipStream_t stream);
int lafs_shard_margin_grad(float* cos, int ld, int B, int S, const int32_t* y_local, const int32_t* y2_local, const float* lam, float s,
                           float m, int margin_type, const float* gmax, const float* Z, float grad_scale, hipStream_t stream);
/* x(f32) [B,3,S,S]: x = lam*x + (1-lam)*flip_batch(x), from a u8 source with (x/255*2-1) folded in (util/mixup_my.py:189-200 on
 * the loader's tensors, train_largescale.py:842-846).  lam_dev != NULL: lambda is read from DEVICE memory when the kernel runs (a
 * captured fine-tune step replays with a new lambda per micro-step); otherwise `lam`. */
int lafs_mixup_normalize(const uint8_t* src_u8, float* dst, int B, int S, float lam, const float* lam_dev, hipStream_t stream);
/* The fused margin-softmax + soft-target CE of lafs_margin_softmax_ce over (row, chunk) workgroups, for the captured fine-tune
 * step: cos(f32) [B, ld] is READ-ONLY, dL/dcos leaves as bf16 in dcos [B, lddc] (pad columns [C, lddc) zeroed) -- the operand of
 * the two class-gradient GEMMs; y2 == NULL: the mixup partner of row b is row B-1-b; lam_dev != NULL: lambda from device memory.
 * row_ws f32 [B], part_ws f32 [B * 32].  Same references as lafs_margin_softmax_ce.  This is lafs_margin_softmax_ce_mix_bf16 with one
 * lambda for the whole batch and eps = 0: the same kernels run. */
int lafs_margin_softmax_ce_bf16(const float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2, float lam,
                                const float* lam_dev, float s, float m, int margin_type, float loss_scale, void* dcos, int lddc,
                                float* loss_out, float* row_ws, float* part_ws, hipStream_t stream);
/* The mixing recipe beyond batch-mode mixup (util/mixup_my.py:27-81 CutMix boxes, :114-187 pair / elem modes, :18-24 label smoothing).
 * One parameter row per sample in DEVICE memory, LAFS_MIX_WORDS 32-bit words each, read when the kernels run (a captured micro-step
 * replays with new parameters):  [0] lambda (f32; after CutMix's area correction), [1] CutMix flag (i32, 0 / 1), [2..5] box yl, yh, xl,
 * xh (i32; rows [yl, yh) x columns [xl, xh)).  The partner of row b is row B-1-b in every mode (:157, :174, :196).
 * lafs_mix_normalize: src u8 [B,3,S,S] -> dst f32, x/255*2-1 folded in.  Flag 0: lam*x[b] + (1-lam)*x[B-1-b] with the arithmetic of
 *   lafs_mixup_normalize (lambda 1: the row passes through); flag 1: x[B-1-b] inside the box, x[b] outside (all three channels). */
enum { LAFS_MIX_LAM = 0, LAFS_MIX_CUT, LAFS_MIX_YL, LAFS_MIX_YH, LAFS_MIX_XL, LAFS_MIX_XH, LAFS_MIX_WORDS };
int lafs_mix_normalize(const uint8_t* src_u8, float* dst, int B, int S, const int32_t* table, hipStream_t stream);
/* lafs_margin_softmax_ce_bf16 with a lambda per row and label smoothing `eps`: lambda of row b = lam_rows[b * lam_stride] (f32 in
 * device memory; lam_stride = 1: a plain array, LAFS_MIX_WORDS: the table above).  Target of row b, never materialised:
 *   y_k = eps/C + (1-eps) (lam_b [k = y1[b]] + (1-lam_b) [k = y2[b]])     (util/mixup_my.py:18-24; equal classes: the summed weight)
 * entering the CosFace margin itself, z_k = s (cos_k - m y_k) (face_pre_pro/ViT_face.py:69-73);  loss_b = lse(z) - sum_k y_k z_k
 * (timm SoftTargetCrossEntropy, train_largescale.py:820) = lse(z) - eps/C sum_k z_k - the two spikes;  dcos = loss_scale/B (softmax - y) s.
 * The (row, chunk) kernels of lafs_margin_softmax_ce_bf16, bf16 dcos [B, lddc] with zeroed pad columns and y2 == NULL convention; with
 * eps = 0 the very same launches run, so with one lambda on every row loss and dcos equal that entry's bit for bit.  margin_type 1
 * (ArcFace) treats the two spikes as that entry point does and requires eps = 0.  row_ws f32 [B]; part_ws f32 [B * 48] (per row and
 * chunk: max, sum exp, and for eps > 0 sum z). */
int lafs_margin_softmax_ce_mix_bf16(const float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2, const float* lam_rows,
                                    int lam_stride, float eps, float s, float m, int margin_type, float loss_scale, void* dcos, int lddc,
                                    float* loss_out, float* row_ws, float* part_ws, hipStream_t stream);
/* AdaFace head (Kim, Jain, Liu, CVPR 2022; PARITY UNPINNED: the reference names it, train_largescale.py:820, util/utils.py:398, and
 * ships no class): a margin pair per row from the embedding's norm, the image-quality proxy.  inv_norm f32 [B] as lafs_l2norm_fwd
 * writes it; state f32 [2] = (batch_mean, batch_std) in DEVICE memory (initially 20, 100), read and written when the kernel runs.
 *   n_b = clip(1 / inv_norm[b], 1e-3, 100);  mean = sum n_b / B;  std = sqrt(sum (n_b - mean)^2 / (B - 1))  (unbiased, two passes);
 *   update = 1: state <- t_alpha (mean, std) + (1 - t_alpha) state, BEFORE it is used;  update = 0: the state is read, not written;
 *   k_b = clip((n_b - batch_mean) / (batch_std + 1e-3) h, -1, 1);  row_margin f32 [B, 2] = (g_ang, g_add) = (-m k_b, m + m k_b).
 * One workgroup, a fixed reduction order (the same bits run to run), no atomics.  B >= 2. */
int lafs_adaface_margins(const float* inv_norm, int B, float* state, float t_alpha, float h, float m, int update, float* row_margin,
                         hipStream_t stream);
/* The (row, chunk) launches of lafs_margin_softmax_ce_mix_bf16 with AdaFace's per-row margins in place of (m, margin_type, eps):
 *   c^ = clamp(c, -1 + 1e-3, 1 - 1e-3) on every class;  on the classes whose target weight is > 0 (both spikes of a mixed row):
 *   z = s (cos(clip(acos c^ + g_ang[b], 1e-3, pi - 1e-3)) - g_add[b]);  elsewhere z = s c^;  loss_b = lse(z) - sum_k y_k z_k;
 *   dcos_k = loss_scale/B (softmax_k - y_k) dz_k/dc_k,  dz/dc = s sin(theta_m) / sin(theta) on a target, s elsewhere, and exactly 0 where
 *   c was clamped or theta_m clipped (the thresholds are the fp32 constants).  No gradient flows into the margins.
 * lambda of row b = lam_rows[b * lam_stride] (device memory; stride 0: one lambda for the batch, 1: an array, LAFS_MIX_WORDS: the
 * table); y2 == NULL: the partner of row b is row B-1-b.  cos is read-only; bf16 dcos [B, lddc], pad columns [C, lddc) zeroed;
 * row_ws f32 [B]; part_ws f32 [B * 32]. */
int lafs_margin_softmax_ce_ada_bf16(const float* cos, int ld, int B, int C, const int32_t* y1, const int32_t* y2, const float* lam_rows,
                                    int lam_stride, const float* row_margin, float s, float loss_scale, void* dcos, int lddc,
                                    float* loss_out, float* row_ws, float* part_ws, hipStream_t stream);
/* dst(i32)[n] = src(i64)[n]: the loader's int64 labels (train_largescale.py:842) into the kernels' index type without an ATen cast */
int lafs_cast_i64_i32(const int64_t* src, int32_t* dst, int n, hipStream_t stream);
/* Patch-vector gradient f32 [B, (S/8)^2, 192] -> image gradient f32 [B, 3, S, S]: the inverse re-indexing of lafs_patchify (the
 * landmark branch differentiates through the patches, face_pre_pro/ViT_face.py:679-711; was a torch permute + copy). */
int lafs_unpatchify_f32(const float* dpatch, int B, int S, int order, float* dimg, hipStream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Frozen landmark CNN, inference only (MobileNetV3-large trunk, face_pre_pro/mobilenet.py:224-313, called by
 * face_landmark_4simmin_glo_loc.forward, face_pre_pro/ViT_face.py:1338-1344).  NHWC bf16 activations, channel counts padded
 * to multiples of 32, BatchNorm folded into (w, b) by the host; the 1x1 convolutions are lafs_gemm_nt(LAFS_EPI_BF16_ACT).
 * act: LAFS_ACT_* (negative = none).
 * ------------------------------------------------------------------------------------------------ */
/* stem: x f32 NCHW [N,3,S,S], w f32 [27][16] (index (c*9+ky*3+kx)*16+o), b f32 [16] -> y bf16 NHWC [N,S/2,S/2,ldy]
 * = act(conv3x3 stride 2 pad 1 + b) in channels 0..15, zeros in 16..ldy-1. */
int lafs_cnn_stem(const float* x, const float* w, const float* b, int N, int S, int act, void* y, int ldy, hipStream_t stream);
/* depthwise k x k (k in {3,5}), stride in {1,2}, pad (k-1)/2: x bf16 [N,H,W,C], w f32 [k*k][C], b f32 [C] -> y bf16
 * [N,ceil(H/stride),ceil(W/stride),C] = act(conv + b).  C % 8 == 0. */
int lafs_cnn_dwconv(const void* x, const float* w, const float* b, int N, int H, int W, int C, int k, int stride, int act,
                    void* y, hipStream_t stream);
/* out(bf16)[n, c] = mean over the HW positions of x bf16 [N,HW,C]  (squeeze; final average pool).  C % 8 == 0, ldo >= C: columns
 * [C, ldo) of out are not written.  Two kernels (one workgroup per image for HW >= 16 and C <= 2048, else one thread per image and
 * 8 channels), both with a fixed order of additions: a repeated call is bit-identical. */
int lafs_cnn_pool(const void* x, int N, int HW, int C, void* out, int ldo, hipStream_t stream);
/* x(bf16)[n,p,c] = act(x[n,p,c] * s(bf16)[n,c]) in place  (excite + the block's non-linearity). */
int lafs_cnn_scale_act(void* x, const void* s, int lds, int N, int HW, int C, int act, hipStream_t stream);

/* Depthwise convolution of the TRAINABLE landmark branch (fine-tune step, nn.Conv2d(C, C, k, stride, (k-1)//2, groups=C,
 * bias=False) of face_pre_pro/mobilenet.py:177-186 and its two gradients), fp32 NCHW.  x [N,C,H,W], w [C,1,k,k],
 * y / dy [N,C,ceil(H/stride),ceil(W/stride)]; k in {3,5}, stride in {1,2}.  bwd_weight ACCUMULATES into dw (zero it first). */
int lafs_dwconv_nchw_fwd(const float* x, const float* w, int N, int C, int H, int W, int k, int stride, float* y, hipStream_t stream);
int lafs_dwconv_nchw_bwd_data(const float* dy, const float* w, int N, int C, int H, int W, int k, int stride, float* dx,
                              hipStream_t stream);
int lafs_dwconv_nchw_bwd_weight(const float* x, const float* dy, int N, int C, int H, int W, int k, int stride, float* dw,
                                hipStream_t stream);

/* BatchNorm2d (+ activation LAFS_ACT_NONE / RELU / HSWISH) of the trainable landmark branch, fp32 NCHW
 * (face_pre_pro/mobilenet.py:104-111,177-190).  x, y, dy, dx [N,C,HW]; stat f32 [2C] receives {mean, rstd} (saved for the
 * backward); sums_ws / dsum f32 [2C] are scratch (dsum returns {dbeta, dgamma} = {sum dz, sum dz*xhat}).
 * training = 1: batch statistics (biased variance) + running-statistics update with `momentum` (unbiased variance), exactly
 * nn.BatchNorm2d.train(); training = 0: running statistics, the backward treats them as constants. */
int lafs_bn_act_fwd_nchw(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float eps,
                         float momentum, int training, int N, int C, int HW, int act, float* sums_ws, float* stat, float* y,
                         hipStream_t stream);
int lafs_bn_act_bwd_nchw(const float* x, const float* dy, const float* stat, const float* gamma, const float* beta, int training,
                         int N, int C, int HW, int act, float* dsum, float* dx, hipStream_t stream);

/* View augmentation of the loader (DataAugmentation_LAFS, lafs_train.py:790-886; Pillow arithmetic, bit-exact):
 * images u8 NCHW [B,3,112,112]; params i32 [B,K,20] records (lafs_cvpr2024_amd/augment.py pack_params: crop box, flags
 * {flip, jitter, gray, solarize}, ColorJitter order + factors, hue shift, box-blur radius/weights); table i32 [113,112,8] =
 * Pillow's bicubic resampling coefficients for every source extent (augment.py coeff_table).
 * views f32 [2K,B,3,112,112]: view 2k = normalised resized crop (+flip) of crop k, view 2k+1 = its colour-augmented twin. */
int lafs_augment_views(const uint8_t* images, const int32_t* params, const int32_t* table, int B, int K, float* views,
                       hipStream_t stream);

/* The DINO-face baseline's views (DataAugmentationDINO, lafs_train.py:743-788: RandomResizedCrop(112 | 48, BICUBIC) :760,767,776,
 * RandomHorizontalFlip + ColorJitter + RandomGrayscale :745-752, utils.GaussianBlur :762,769,778, utils.Solarization :770,
 * ToTensor + Normalize :753-756; Pillow arithmetic, bit-exact).  ONE view per crop, the whole colour chain on every view.
 * images u8 NCHW [B,3,112,112]; params i32 [B,2+n_local,20], the records of lafs_augment_views (crop 0, 1 = globals, 2.. = locals);
 * table_g i32 [113,112,8] = the table of lafs_augment_views; table_l i32 [113,48,table_l_words] = the same for output size 48:
 * per output index (first source index, taps, coefficients), table_l_words >= 2 + the most taps (10 for 112 -> 48);
 * mean_std: 6 HOST floats {mean r,g,b, std r,g,b} of Normalize, (v / 255.f - mean) / std in fp32, each operation rounded.
 * globals f32 [2B,3,112,112]: crop k of image b -> row k*B + b; locals f32 [n_local*B,3,48,48]: crop 2+k of image b -> row
 * k*B + b (the crop-major input buffers of the pre-training engine).  Two launches of 1024-thread workgroups, 2B (112 KB of LDS each)
 * and n_local*B (30 KB each); n_local = 0 launches the globals only (table_l and locals may then be null). */
int lafs_dino_views(const uint8_t* images, const int32_t* params, const int32_t* table_g, const int32_t* table_l, int table_l_words,
                    int B, int n_local, const float* mean_std, float* globals, float* locals, hipStream_t stream);

/* RandAugment of the fine-tune loader (reference util/rand_aa_face.py:606-672 as FaceDataset builds it, face_pre_pro/
 * dataloader_web.py:240-243 -- 'rand-m1-mstd0.5-inc1', train_largescale.py:506 -- applied per decoded sample at
 * dataloader_web.py:342-346 / image_iter.py:324-329; Pillow arithmetic, bit-exact).  One record per image and layer, sampled on
 * the host in the reference's random order (lafs_cvpr2024_amd/randaug.py):
 *   op        -1 = layer not applied; 0..12 = AutoContrast, Equalize, Invert, Rotate, PosterizeIncreasing, ColorIncreasing,
 *             ContrastIncreasing, BrightnessIncreasing, SharpnessIncreasing, ShearX, ShearY, TranslateXRel, TranslateYRel
 *             (the order of _RAND_INCREASING_TRANSFORMS :560-576); 13 / 14 / 15 = the transposes Image.rotate substitutes for 180 / 90 /
 *             270 degrees
 *   resample  2 = PIL BILINEAR, 3 = BICUBIC (geometric ops)       iarg   Posterize: the byte mask ~(2^(8-bits) - 1)
 *   farg      enhancement factor of Color / Contrast / Brightness / Sharpness (Image.blend's float alpha)
 *   m[6]      the AFFINE matrix handed to Image.transform (output pixel centre -> source position), double precision
 * images / out: u8 [B, H, W, 3] (chw = 0) or [B, 3, H, W] (chw = 1), 3 <= H, W and H * W <= 112 * 112; out may alias images. */
typedef struct lafs_randaug_op {
  int32_t op, resample, iarg;
  float farg;
  double m[6];
} lafs_randaug_op;
int lafs_randaug_apply(const uint8_t* images, uint8_t* out, const lafs_randaug_op* records, int B, int H, int W, int layers, int chw,
                       hipStream_t stream);

/* The torchvision tensor chain of the fine-tune loader (reference image_iter.py:214-219, applied at :349-351 after RandAugment):
 * Compose([RandomResizedCrop(112, scale=(0.9, 1.0)), ColorJitter(0.1, 0.1, 0.1, 0.1), RandomErasing(scale=(0.02, 0.1))]) on the
 * uint8 CHW tensor.  PARITY UNPINNED (restated from torchvision 0.9.1; torchvision is not installed): the arithmetic is that of
 * 0.9.1's functional_tensor as the installed torch evaluates it on the CPU, bit-exact against tests/facedataset_tv_oracle.py.
 * One 80-byte record per image, drawn on the host with torchvision's own torch calls (lafs_cvpr2024_amd/face_tensor_aug.py):
 *   crop_i, crop_j, crop_h, crop_w   RandomResizedCrop.get_params box in the source; resampled to S x S as F_t.resize does it
 *                                    (float32 bilinear interpolate, align_corners=False, round half to even, uint8 cast)
 *   order[4]                         ColorJitter.get_params fn_idx: 0 brightness, 1 contrast, 2 saturation, 3 hue, applied in turn
 *   brightness, brightness_c         _blend weights r and 1 - r (float32 of the Python doubles) of adjust_brightness (b = 0),
 *   contrast, contrast_c             adjust_contrast (b = mean grayscale) and
 *   saturation, saturation_c         adjust_saturation (b = uint8 grayscale)
 *   hue                              adjust_hue factor in [-0.1, 0.1] (float32): rgb2hsv, h = (h + f) % 1, hsv2rgb, truncating cast
 *   erase                            1: RandomErasing applies, the box (erase_i, erase_j, erase_h, erase_w) of the S x S result is
 *   erase_i, erase_j, erase_h, erase_w  set to 0 (value=0); 0: not applied, or no box was found in 10 tries
 * images u8 [B,3,H,W], 3 <= H, W, H * W <= 112^2; out u8 [B,3,S,S], 3 <= S <= 112; out may alias images when H = W = S.
 * Boxes outside the image are clamped into it (the host validates them first). */
typedef struct lafs_face_tensor_aug_rec {
  int32_t crop_i, crop_j, crop_h, crop_w;
  int32_t order[4];
  float brightness, brightness_c, contrast, contrast_c, saturation, saturation_c, hue;
  int32_t erase, erase_i, erase_j, erase_h, erase_w;
} lafs_face_tensor_aug_rec;
int lafs_face_tensor_aug(const uint8_t* images, uint8_t* out, const lafs_face_tensor_aug_rec* recs, int B, int H, int W, int S,
                         hipStream_t stream);

/* JPEG decode of the RecordIO loaders (the reference decodes with mx.image.imdecode in its DataLoader workers, image_iter.py:300-306;
 * this project's CPU path is Pillow).  libjpeg's integer arithmetic, bit-exact against Pillow (libjpeg-turbo): Huffman decoding,
 * dequantisation, jidctint "islow", "fancy" h2v1 / h2v2 chroma upsampling (replication for planes of width <= 2), YCbCr -> RGB.
 * Accepted: SOF0 / SOF1 with 8-bit samples, one scan (Ss = 0, Se = 63, Ah = Al = 0), one component (written to all three planes)
 * or three read as YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, restart intervals, 1 <= W, H <= LAFS_JPEG_MAX_DIM.
 * The host walks the markers (lafs_cvpr2024_amd/jpeg.py parse / pack) and hands over, per image, one record and the bytes of its scan:
 *   data_off, data_len   the entropy-coded bytes (stuffed FF 00 and RSTn markers included, up to but excluding the marker that ends
 *                        the scan) inside `stream`
 *   table_off            byte offset inside `tables` of this image's LAFS_JPEG_TABLE_BYTES block: 4 x 64 uint16 quantiser entries
 *                        (little-endian, DQT = zigzag order, slot = table id) followed by the Huffman tables DC 0, DC 1, AC 0, AC 1,
 *                        each 16 BITS bytes + 256 HUFFVAL bytes, zero-padded; images with the same tables may share a block
 *   width, height        must equal the W, H of the call
 *   ncomp                1 or 3;   hs, vs  sampling factors (1x1 for one component);   tq, td, ta  table ids per component
 *   restart_interval     MCUs between RSTn markers, 0 = none
 * out u8 [B,3,H,W]; status i32 [B]: 0 = decoded, otherwise a sum of LAFS_JPEG_ST_* and out[b] is undefined (but only out[b] and
 * the image's own workspace slice were written; a record that fails validation writes nothing).  The kernel trusts no field of a
 * record, table or stream: every loop is bounded by the block count of a W x H image, reads are clamped to data_len.
 * workspace: lafs_jpeg_workspace_bytes(B, H, W) bytes, 16-byte aligned (-1 for sizes outside the limits). */
#define LAFS_JPEG_MAX_DIM 1024
#define LAFS_JPEG_TABLE_BYTES 1600
enum { LAFS_JPEG_ST_RECORD = 1,   /* record refused: size, sampling, offsets */
       LAFS_JPEG_ST_OVERRUN = 2,  /* bits were needed past the end of the scan or past a marker */
       LAFS_JPEG_ST_CODE = 4,     /* no Huffman code matched within 16 bits */
       LAFS_JPEG_ST_COEF = 8,     /* a run went past coefficient 63, or a DC value left the int16 range */
       LAFS_JPEG_ST_RESTART = 16  /* the expected RSTn marker was not there */ };
typedef struct lafs_jpeg_image {
  int64_t data_off;
  int32_t data_len, table_off;
  int32_t width, height, ncomp, restart_interval;
  uint8_t hs[3], vs[3], tq[3], td[3], ta[3];
  uint8_t pad[17];
} lafs_jpeg_image;
int64_t lafs_jpeg_workspace_bytes(int B, int H, int W);
int lafs_jpeg_decode(const uint8_t* stream, int64_t stream_bytes, const lafs_jpeg_image* images, const uint8_t* tables,
                     int64_t table_bytes, int B, int H, int W, uint8_t* out, int32_t* status, void* workspace, hipStream_t stream_id);

/* Face verification of the fine-tune loop (reference util/utils.py:292-397 perform_val, util/verification.py:38-87 calculate_roc,
 * :224-234 calculate_accuracy; called every VER_FREQ optimizer steps by train_largescale.py:925-959).
 * lafs_eval_flip_normalize: src u8 [B,3,S,S] -> dst f32 [2B,3,S,S]; rows 0..B-1 = x / div * mul + add, every operation rounded on its
 *   own (div 255, mul 1, add -0.5 is the reference's `batch/255.0-0.5` of utils.py:314 as torch evaluates it on the CPU; div 1,
 *   mul 2/255, add -1 is the training feed of lafs_mixup_normalize); rows B..2B-1 = the same images mirrored along W
 *   (load_bin's mx.ndarray.flip(axis=2) on CHW, utils.py:38-41).  S % 16 == 0, both operands 16-byte aligned.
 * lafs_verify_tail: feat f32 [2B, ldf] = the trunk's embeddings of those 2B rows (row B + i mirrors row i); pair j of the batch is
 *   images 2j, 2j+1 = global pair pair0 + j of n_pairs.  Per pair, in fp64: norms[img] = ||feat_orig||, norms[2 n_pairs + img] =
 *   ||feat_flip|| (utils.py:377-384, XNorm), e = feat_orig + feat_flip L2-normalised (utils.py:386-387, sklearn normalize),
 *   dist = sum (e1 - e2)^2 (verification.py:51-52) -> dist[pair] and the normalised e -> emb f32 [2 n_pairs, D] when non-NULL;
 *   k0 = #{k : thresholds[k] <= dist} (binary search of the ascending fp64 table, NaN -> n_thr) and
 *   hist i32 [n_folds][2][n_thr + 1][fold(pair)][issame[pair] != 0][k0] += 1, fold f = [fold_start[f], fold_start[f + 1]).
 *   The pair counts with dist < thresholds[k] are the prefix sums of hist over k0 <= k.  Integer atomics: deterministic.
 *   B even, D <= 1024, n_thr * 8 + n_folds * 2 * (n_thr + 1) * 4 <= 64 KiB. */
int lafs_eval_flip_normalize(const uint8_t* src_u8, float* dst, int B, int S, float div, float mul, float add, hipStream_t stream);
int lafs_verify_tail(const float* feat, int ldf, int B, int D, int pair0, int n_pairs, const double* thresholds, int n_thr,
                     const int32_t* fold_start, int n_folds, const uint8_t* issame, int32_t* hist, double* norms, double* dist,
                     float* emb, hipStream_t stream);

/* IJB-B / IJB-C template verification (csrc/ijb.hip; reference IJB_evaluation.py).
 * lafs_ijb_align_flip_normalize (:198-247, Embedding.get's cv2.warpAffine + np.fliplr and forward_db's div_(255).sub_(0.5)):
 *   src u8 = B loose crops packed back to back as HWC RGB, image b at byte offsets[b] with hw[2b], hw[2b+1] = (H, W); inv_maps f32
 *   [B,6] = the INVERSE map, output pixel (x, y) -> source (m0 x + m1 y + m2, m3 x + m4 y + m5).  dst f32 [2B,3,S,S]: rows 0..B-1 the
 *   aligned crops scaled as x / div * mul + add (lafs_eval_flip_normalize's arithmetic), rows B..2B-1 the same mirrored along W;
 *   aligned_u8 u8 [B,3,S,S] (may be NULL) the aligned crops.  Float32 bilinear, four taps, a tap outside the image reads 0 (border
 *   value 0), rounded to nearest even; the operation order is fixed in ijb.hip.  Reads outside [src, src + src_bytes) are refused
 *   per image (such an image comes out as zeros).  OpenCV interpolates in fixed point on a 1/32 pixel grid: parity unpinned.
 * lafs_ijb_template_pool (:731-751 and :501-535 image2template_feature): feats f32 [n_images, ldf] rows [emb(orig) | emb(flip)],
 *   faceness f32 [n_images]; order i32 [n_images] = the images sorted by (template, media, index); media m holds order[media_start[m]
 *   .. media_start[m+1]), template t holds media [template_start[t], template_start[t+1]).  Per column in float32: x = (a + b) * s
 *   (b only when flip, s only when detector_score), sequential adds inside a media, one division by the count when it exceeds 1
 *   (np.mean), sequential adds over the media (np.sum) -> sums f32 [n_templates, D], bit for bit numpy's; then in float64 the row
 *   divided by its L2 norm, a zero row left as it is (sklearn.preprocessing.normalize) -> unit f64 [n_templates, D].  D <= 1024.
 * lafs_ijb_pair_scores (:541-567 verification): scores[p] = sum_d unit[idx1[p], d] * unit[idx2[p], d] in float64; an index outside
 *   [0, n_templates) scores NaN. */
int lafs_ijb_align_flip_normalize(const uint8_t* src_u8, int64_t src_bytes, const int64_t* offsets, const int32_t* hw,
                                  const float* inv_maps, int B, int S, float div, float mul, float add, float* dst, uint8_t* aligned_u8,
                                  hipStream_t stream);
int lafs_ijb_template_pool(const float* feats, int ldf, const float* faceness, int n_images, const int32_t* order,
                           const int32_t* media_start, int n_media, const int32_t* template_start, int n_templates, int D, int flip,
                           int detector_score, float* sums, double* unit, hipStream_t stream);
int lafs_ijb_pair_scores(const double* unit, int n_templates, int D, const int32_t* idx1, const int32_t* idx2, int64_t n_pairs,
                         double* scores, hipStream_t stream);

/* IJB-B / IJB-C 1:N identification: every probe template against every gallery template, top-k and three scalars per probe; the
 * n_probes x n_gallery scores are never stored (csrc/ijb.hip).  No counterpart in the reference.
 *   unit f64 [n_templates, D] (lafs_ijb_template_pool's rows), D in [1, 1024]; probe_idx i32 [n_probes] and gallery_idx i32 [n_gallery]
 *   name rows of unit (nothing is gathered; a row may repeat, no order is assumed); mate i32 [n_probes] = the POSITION in gallery_idx
 *   of the probe's subject, -1: none (a value outside [-1, n_gallery) is treated as -1); k in [1, 64].
 * Score: score(i, j) = the float64 dot product of rows probe_idx[i] and gallery_idx[j].  Its order of summation is a function of D
 *   alone (column blocks of 4 in ascending order, zeros up to the next multiple of 32): it does not depend on where the rows sit in
 *   a tile, a workgroup or either list, on the launch geometry, or on whether the pair is the mate -- the same two rows give the same
 *   64 bits wherever they appear.
 * Ranking order of the gallery positions of one probe: larger score first; equal scores: smaller position first; a NaN score (a
 *   non-finite row, e.g. from non-finite image features) after every number, among NaNs the smaller
 *   position first.
 * top_score f64 / top_idx i32 [n_probes, k]: the first k entries of that order (positions in gallery_idx); when n_gallery < k the
 *   tail is idx -1, score NaN.  mate_score f64 [n_probes] = score(i, mate[i]), NaN without a mate.  mate_rank i32 [n_probes] = the
 *   number of gallery positions that precede the mate in the ranking order over the WHOLE gallery (0: a rank-1 hit), -1 without a
 *   mate.  best_nonmate f64 [n_probes] = the first score of the ranking order with position mate[i] left out, NaN if nothing is left.
 * A probe index outside [0, n_templates) gives that probe idx -1, NaN scores and rank -1; a gallery index outside it scores NaN
 *   against every probe (lafs_ijb_pair_scores' rule), so it ranks last.  Nothing outside unit is read.
 * lafs_ijb_search_workspace returns the bytes of workspace the search needs (0 in this design: workspace may then be NULL). */
int64_t lafs_ijb_search_workspace(int n_probes, int n_gallery, int k);
int lafs_ijb_search(const double* unit, int n_templates, int D, const int32_t* probe_idx, int n_probes, const int32_t* gallery_idx,
                    int n_gallery, const int32_t* mate, int k, double* top_score, int32_t* top_idx, double* mate_score,
                    int32_t* mate_rank, double* best_nonmate, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Weighted k-NN on frozen float32 features (csrc/knn.hip): every query row against every bank row, the first k bank positions per
 * query, then DINO's exp(score / T)-weighted class vote.  The n_query x n_bank scores are never stored.  No counterpart in the
 * reference; the vote restates the formula of DINO's eval_knn.py knn_classifier.
 *   bank f32 [n_bank, ldb] and query f32 [n_query, ldq], of which the first D columns are used (only those are read); D in
 *   [1, 1024], k in [1, 256], bank_pos0 >= 0 and bank_pos0 + n_bank < 2^31.  Alignment rule: ldb % 4 == 0, ldq % 4 == 0 and both
 *   base pointers 16-byte aligned (rows are read 16 bytes at a time).  Rows are taken as given: the host normalises them.
 * Score: the float32 dot product on v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain from 0: columns in ascending order, zeros from D
 *   up to the next multiple of 32.  The order is a function of D alone: the same two rows give the same 32 bits wherever they sit
 *   -- in a tile, a workgroup, a bank chunk or a split.  A NaN score is returned as the canonical quiet NaN.
 * Ranking order of one query's bank positions (bank_pos0 + row): larger score first; equal scores: smaller position first; NaN after
 *   every number, among NaNs the smaller position first.
 * top_score f32 / top_idx i32 [n_query, k]: the first k entries of that order; with fewer than k candidates the tail is idx -1,
 *   score NaN.  exclude i32 [n_query] or NULL: the one position never returned for that query (-1: none) -- leave-one-out when the
 *   bank holds the queries.
 * merge != 0: top_score / top_idx already hold a valid result over OTHER positions (earlier bank chunks); this call's candidates are
 *   merged into it in the same order.  A bank presented in any number of chunks, in any chunk order, gives the same bits as one call.
 * splits: the bank of one call is divided among `splits` workgroups per 64 queries (0: chosen from n_query, n_bank and the CU count;
 *   at most 32 and at most one per 128 bank rows are used); partial lists go to `workspace` and a merge pass combines them.  The
 *   result is bit-identical for every value.  lafs_knn_workspace returns the bytes lafs_knn_search needs for the same four
 *   arguments (0 when one split runs: the lists are then the output rows and workspace may be NULL); a shorter workspace is refused.
 * Every refusal (negative code) happens before anything is launched: nothing is written.
 * lafs_knn_vote: for every query and every ks[i] (HOST array of n_ks <= 8 values, ascending, each in [1, k]) each of the first
 *   ks[i] list entries with 0 <= idx < n_label gives exp(score / temperature) to class bank_label[idx] (bank_label i32 [n_label] on
 *   the device, indexed by position; any non-negative int32).  A class's vote is the float32 sum of its entries in list order.
 *   Classes are ordered by larger vote first, then smaller label; pred i32 / vote f32 [n_ks, n_query, 5] hold the first five,
 *   unused slots -1 and 0.  Only the at most k retrieved labels are touched: the cost does not depend on the number of classes. */
int64_t lafs_knn_workspace(int n_query, int64_t n_bank, int k, int splits);
int lafs_knn_search(const float* bank, int ldb, int64_t n_bank, int64_t bank_pos0, const float* query, int ldq, int n_query, int D, int k,
                    const int32_t* exclude, int merge, int splits, float* top_score, int32_t* top_idx, void* workspace,
                    size_t workspace_bytes, hipStream_t stream);
int lafs_knn_vote(const float* top_score, const int32_t* top_idx, int n_query, int k, const int32_t* bank_label, int64_t n_label,
                  const int32_t* ks, int n_ks, float temperature, int32_t* pred, float* vote, hipStream_t stream);

/* Softmax cross-entropy of plain logits with the rank of the target and, optionally, the bf16 gradient (csrc/linear_probe.hip): the
 * loss of the linear probe on frozen features, the trained half of DINO's evaluation pair (eval_linear.py; no counterpart in the
 * reference).  logits f32 [B, ld], READ-ONLY, of which the first C columns are classes; y i32 [B] on the device.  For a row with
 * 0 <= y[b] < C, z = logits[b]:
 *   row_loss[b] = logsumexp_j(z_j) - z_y      the row's maximum subtracted inside every exponential, sums in fp32;
 *   row_rank[b] = #{ j < C : z_j > z_y or (z_j == z_y and j < y) }: top-1 is rank == 0, top-5 rank < 5, nothing is sorted, and the tie
 *                 rule makes the rank a function of the logits alone (comparisons of f32 values: the rank is exact);
 *   dlogits(bf16)[b, j] = bf16(grad_scale (softmax(z)_j - [j == y]))   for j < C, zero for C <= j < lddl: the buffer is the bf16
 *                 operand of lafs_gemm_tn_acc as it stands.  dlogits_bf16 == NULL: no gradient is formed and nothing of it written.
 * y[b] == -1: the row has no target (the padding of a short last batch): loss 0, rank -1, a zero gradient row.  Any other label outside
 * [0, C) cannot be caught on the host: loss NaN, rank -2, a zero gradient row, nothing written outside the row.
 * 1 <= B <= 65535, 1 <= C <= ld; lddl >= C, lddl % 8 == 0 and dlogits 16-byte aligned.  Rows that start on a 16-byte boundary
 * (ld % 4 == 0 and an aligned base) are read 16 bytes at a time throughout; others take a scalar head up to the boundary and a scalar
 * tail.  (row, chunk of 4096 columns) partials, a per-row fold, then the (row, chunk) gradient pass: every sum in a fixed order, no
 * atomics, the same bits on every call.  Bytes per call: 4 B C without the gradient, 8 B C + 2 B lddl with it (the gradient pass
 * reads the logits a second time).  ws: lafs_softmax_ce_rank_workspace_bytes(B, C) bytes, 4-byte aligned, contents irrelevant on entry. */
int64_t lafs_softmax_ce_rank_workspace_bytes(int B, int C);
int lafs_softmax_ce_rank(const float* logits, int ld, int B, int C, const int32_t* y, float grad_scale, void* dlogits_bf16, int lddl,
                         float* row_loss, int32_t* row_rank, float* ws, hipStream_t stream);

/* KoLeo regulariser (csrc/koleo.hip): the Kozachenko-Leonenko differential-entropy term DINOv2 adds to the DINO loss, which pushes
 * every row of a batch away from its nearest neighbour on the sphere.  No counterpart in the reference; restated from DINOv2's
 * published KoLeoLoss (PARITY UNPINNED).  x f32 [n_groups * rows, ldx], READ-ONLY, of which the first D columns are features; group g
 * owns rows [g rows, (g + 1) rows) of x and of dx, and neighbours are never searched across groups.  For one group of n = rows rows:
 *   xh_i = x_i / max(||x_i||, eps)                                    F.normalize(x, p=2, dim=-1, eps=eps)
 *   I(i) = argmax over j != i of <xh_i, xh_j>                         the lowest j among exactly equal values; constant for the gradient
 *   v_i  = xh_i - xh_I(i) + eps,  d_i = ||v_i||                       nn.PairwiseDistance(2, eps): eps added to every element
 *   L    = -(1 / n) sum_i log(d_i + eps)
 *   c_i  = -(1 / n) v_i / (d_i (d_i + eps)),  g_j = c_j - sum over {i : I(i) = j} of c_i, in ascending i
 *   dL/dx_j = (g_j - xh_j <xh_j, g_j>) / ||x_j|| where ||x_j|| >= eps, g_j / eps below (the gradient of the clamp)
 * (The search ranks row i's candidates by <x_i, x_j> / max(||x_j||, eps): the cosine times ||x_i||, constant over j.  A row is never its
 * own candidate.)  Exact duplicates are legal: then v_i = eps in every element, d_i = eps sqrt(D), loss and gradient large but finite.
 * Outputs: loss[g] = L of group g, unscaled;  nn i32 [n_groups * rows] (may be NULL) = I(i) as a row index INSIDE the group;
 * dx (may be NULL: forward only) [n_groups * rows, lddx]: dx[r, :D] = (accumulate ? dx[r, :D] : 0) + grad_scale dL_g/dx_r -- columns
 * >= D and rows outside the call are not touched.  All arithmetic is fp32 and no 16-bit value is stored.  Every sum over D has one
 * order for every row, nothing is an atomic (the scatter of c_i is a gather over the group's neighbour list): identical rows give
 * exactly equal scores, and two calls on equal inputs give equal bits.  Two launches.
 * Accepted: n_groups >= 1, 2 <= rows <= 1024, 4 <= D <= 1024, D % 4 == 0, ldx, lddx >= D and % 4 == 0, eps > 0, x, dx and ws 16-byte
 * aligned; anything else (rows == 1 included) returns a negative code before any launch.  ws: lafs_koleo_workspace_bytes(n_groups,
 * rows, D) bytes (-1 for a shape that is not accepted), contents irrelevant on entry. */
int64_t lafs_koleo_workspace_bytes(int n_groups, int rows, int D);
int lafs_koleo_fwd_bwd(const float* x, int ldx, int n_groups, int rows, int D, float eps, float grad_scale,
                       float* loss /* [n_groups], written */, int32_t* nn /* [n_groups*rows], written; may be NULL */,
                       float* dx /* may be NULL: forward only */, int lddx, int accumulate, void* ws, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * TRAINABLE landmark CNN of the fine-tune step (csrc/landmark_train.hip; reference face_pre_pro/mobilenet.py:224-313 trained through
 * ViT_face.py:679-711 by train_largescale.py:785-891).  Activations are NHWC bf16 [N H W, ld] matrices, ld = channel count padded
 * to a multiple of 32 with the pad channels exactly zero; 1x1 convolutions and their two gradients are lafs_gemm_nt / lafs_wgrad
 * calls on those matrices; the rest is below.  `C` is the true channel count, `ld*` the padded row strides.
 * ------------------------------------------------------------------------------------------------------------------------ */
/* 3x3 stride-2 pad-1 stem as im2col rows: x f32 NCHW [N,3,S,S] -> P bf16 [N (S/2)^2, 32], column (c, ky, kx), columns 27..31 zero. */
int lafs_cnn_im2col_stem(const float* x, int N, int S, void* P, hipStream_t stream);
/* Round 4: every 16-bit tensor of this plan (activations, operand images, activation gradients -- "bf16" in the comments below is
 * historical) is IEEE fp16, the format of the reference's autocast run (train_largescale.py:803-804); its GEMMs are lafs_gemm_nt
 * with operand_f16 = 1 and lafs_wgrad_f16.  Activation gradients are scaled by a per-call power of two derived on the device
 * (lafs_cnn_grad_scale) and un-scaled where they leave the 16-bit domain (grad_scale arguments below; NULL = no scaling).
 * nn.BatchNorm2d in TRAINING mode over the rows of x fp16 [R, ldx]:
 *   lafs_cnn_bn_stats : sums(f64)[0..C) += column sums, sums[C..2C) += column sums of squares (caller zeroes `sums`); fp64: mean and
 *                       E[x^2] - mean^2 are formed in double, the order of the atomics stays below fp32 resolution;
 *   lafs_cnn_bn_apply : y = act((x - mean) rstd gamma + beta) (+ resid), biased batch variance; stat(f32)[2C] = {mean, rstd} for the
 *                       backward; running_mean / running_var (NULL or both) get the momentum update with the unbiased variance;
 *   lafs_cnn_bn_bwd   : dz = (dy + add_nc[n, c] / HW) act'(z) with z recomputed from x; dx(fp16) = gamma rstd (dz - mean(dz) -
 *                       xhat mean(dz xhat)); dgamma += sum dz xhat / scale, dbeta += sum dz / scale (arena gradients, may be NULL);
 *                       dsums(f64)[2C] = caller-zeroed scratch.  add_nc fp16 [N, ldadd] (the squeeze-excite pooling gradient) or NULL.
 * Contracts the kernel tests hold (tests/test_gpu_cnn_kernels.py): these three entry points accept any C <= ld (C % 8 != 0 included;
 * only the strides must be multiples of 8); sums / dsums ACCUMULATE (what the buffer held enters the statistics, and dx of the
 * same call); dgamma / dbeta accumulate; y and dx are written over all ld* columns with the pad channels [C, ld*) exactly zero
 * (y whatever the inputs hold there, dx given finite x and dy there); columns of x / dy / resid / add_nc at or beyond the output's
 * row stride are not read.  The fp64 atomics make the sums order-dependent at the 2^-52 level; stat, y and dx are functions of the
 * sums handed in. */
int lafs_cnn_bn_stats(const void* x, int ldx, int64_t R, int C, double* sums, hipStream_t stream);
int lafs_cnn_bn_apply(const void* x, int ldx, int64_t R, int C, const double* sums, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, int act, const void* resid, int ldr, void* y, int ldy,
                      float* stat, hipStream_t stream);
int lafs_cnn_bn_bwd(const void* dy, int lddy, const void* x, int ldx, int64_t R, int C, const float* stat, const float* gamma,
                    const float* beta, int act, const void* add_nc, int ldadd, int HW, double* dsums, void* dx, int lddx,
                    float* dgamma, float* dbeta, const float* grad_scale, hipStream_t stream);
/* nn.BatchNorm2d in EVAL mode (a model.eval() forward that is still differentiated, face_pre_pro/ViT_face.py:679-711 under
 * train_largescale.py's test-time paths): lafs_cnn_bn_eval_sums writes the sums a batch with exactly the running statistics would have
 * (sums[c] = R mean, sums[C + c] = R (var + mean^2), fp64), so that lafs_cnn_bn_apply (running_mean = NULL: no update) normalises with
 * them; lafs_cnn_bn_bwd_eval is lafs_cnn_bn_bwd with the statistics as constants: dx = gamma rstd dz, same dgamma / dbeta. */
int lafs_cnn_bn_eval_sums(const float* running_mean, const float* running_var, int64_t R, int C, double* sums, hipStream_t stream);
int lafs_cnn_bn_bwd_eval(const void* dy, int lddy, const void* x, int ldx, int64_t R, int C, const float* stat, const float* gamma,
                    const float* beta, int act, const void* add_nc, int ldadd, int HW, double* dsums, void* dx, int lddx,
                    float* dgamma, float* dbeta, const float* grad_scale, hipStream_t stream);
/* Loss scaling and overflow guard of the fp16 backward -- the reference's torch.cuda.amp.GradScaler (train_largescale.py:739,
 * 803-804, 867-880: scale, skip the step on inf / NaN, back the scale off, grow it again) decided on the device, so that a captured
 * step needs no host round trip.
 *   lafs_cnn_grad_scale: scale(f32, device)[0..1] = {s, 1/s}, s = the power of two <= target / max |g|, clamped to [2^-24, 2^24]
 *     (1 for an all-zero gradient).  has_state != 0: scale is the 8-float state {s, 1/s, target, found_inf, skipped, clean, -, -}:
 *     the target is state[2] when that is > 0 (else the argument), and found_inf is RESET to "g itself holds inf / NaN".
 *   lafs_cnn_grad_guard (after the backward, over the CNN's gradient range of the arena): found_inf |= any non-finite entry;
 *     found_inf: the range is zeroed (this accumulation window's CNN update is dropped; AdamW's moments stay finite), target
 *     halves (>= 1), skipped += 1; otherwise 2000 clean backwards in a row double the target again (<= target_max).
 *     DEVIATION from GradScaler, by design of this guard: it runs once per MICRO-step and covers the landmark CNN's range only --
 *     (a) with acc_step > 1 an overflow zeroes what earlier micro-steps of the window accumulated there and later ones still add
 *     to it, so the optimizer then applies a partial CNN gradient instead of skipping; (b) the optimizer step itself is never
 *     skipped: AdamW still decays the CNN's weights and moments, and the ViT / margin-head ranges (computed in bf16 with fp32
 *     accumulation, which cannot overflow where fp16 does) update normally, whereas the reference's scaler.step skips the whole
 *     step for every parameter (train_largescale.py:878-880); (c) in data-parallel runs only the overflowing rank zeroes its share
 *     before the all-reduce.  An overflow has not been observed in any test or benchmark run (state[4] == 0 throughout).
 * lafs_cnn_cast_pad_f16: dst(fp16)[r, c] = src(f32)[r, c] * scale[0], pad columns [cols, ld) zero.
 * lafs_cnn_cast_f16_f32: dst(f32)[i] = src(fp16)[i]. */
int lafs_cnn_grad_scale(const float* g, int64_t n, float target, float* scale, int has_state, hipStream_t stream);
int lafs_cnn_grad_guard(float* grad, int64_t n, float* state, float target_max, hipStream_t stream);
int lafs_cnn_cast_pad_f16(const float* src, int rows, int cols, void* dst, int ld, const float* scale, hipStream_t stream);
int lafs_cnn_cast_f16_f32(const void* src, float* dst, int64_t n, hipStream_t stream);
/* Depthwise k x k convolution (k in {3,5}, stride in {1,2}, pad (k-1)/2, no bias) on NHWC bf16.  w = tap-major fp32 image [k*k][ld] of
 * the module's [C][1][k][k] tensor (lafs_cnn_dw_layout_table: table[8 e ..] = {src offset, C, k*k, dst offset, ld}, 256 elements per
 * workgroup); forward; backward = dx(bf16) and dw(f32, += into a tap-major image [k*k][ld] that lafs_cnn_unpad_add_table folds,
 * transposed, into the arena).  y and dx cover all ld channels (pad channels zero given zero pads in x, dy and w); dw is touched in
 * columns [0, C) only, by fp32 atomics (one per tap, channel and slab of >= 1024 output pixels): not bitwise repeatable. */
int lafs_cnn_dw_layout_table(const float* master, float* dst, const int64_t* table, const int32_t* starts, int n_entries, int n_blocks,
                             hipStream_t stream);
int lafs_cnn_dwconv_train_fwd(const void* x, const float* w, int N, int H, int W, int ld, int C, int k, int stride, void* y,
                              hipStream_t stream);
int lafs_cnn_dwconv_train_bwd(const void* x, const void* dy, const float* w, int N, int H, int W, int ld, int C, int k, int stride,
                              void* dx, float* dw, hipStream_t stream);
/* out(bf16)[n, c] = mean over the HW rows of image n (squeeze / final average pool), one workgroup per image. */
int lafs_cnn_pool_train(const void* x, int N, int HW, int ld, void* out, int ldo, hipStream_t stream);
/* Squeeze-excite: out = act(z gate[n, c]) (z kept); backward: ds = dout act'(z gate), dz = ds gate, dgate(f32)[n, c] = sum_p ds z. */
int lafs_cnn_scale_act_out(const void* z, const void* s, int lds_, int N, int HW, int ld, int act, void* out, hipStream_t stream);
int lafs_cnn_se_bwd(const void* dout, const void* z, const void* gate, int ldg, int N, int HW, int ld, int act, void* dz, float* dgate,
                    int lddg, hipStream_t stream);
/* out(bf16)[i] = dy[i] act'(.) from the POST-activation value y (relu, h-sigmoid: the squeeze-excite FCs); dy f32 or bf16. */
int lafs_cnn_act_bwd_post(const float* dy_f32, const void* dy_bf16, const void* y, int64_t n, int act, void* out, hipStream_t stream);
/* dx[n, p, c] = dfeat[n, c] / HW: backward of the final average pool. */
int lafs_cnn_pool_bwd(const void* dfeat, int ldf, int N, int HW, int ld, void* dx, hipStream_t stream);
/* Padded bf16 operand copies of fp32 arena tensors, ONE launch: table(i64, device)[8 e ..] = {src offset, rows, cols, dst offset,
 * dst ld, transpose, padded rows, 0}; starts(i32)[e] = first workgroup of entry e (1024 destination elements per workgroup). */
int lafs_cnn_pad_cast_table(const float* master, void* dst, const int64_t* table, const int32_t* starts, int n_entries, int n_blocks,
                            hipStream_t stream);
/* Padded fp32 weight gradients folded into the arena, ONE launch: table[8 e ..] = {src offset, rows, cols, src ld, grad offset,
 * transpose, ...}; 256 elements per workgroup.  transpose: the source image is [cols][ld] (tap-major depthwise gradients). */
int lafs_cnn_unpad_add_table(const float* padded, float* grad, const int64_t* table, const int32_t* starts, int n_entries, int n_blocks,
                             const float* grad_scale, hipStream_t stream);
/* Backward of theta = (t - min) / (max - min) * 111 per image (ViT_face.py:698-706), incl. the paths through min and max: with equal
 * extrema the FIRST occurrence takes the gradient, as torch.min / torch.max select.  n = 2 n_full > 1; fixed order, bit-identical
 * on a repeated call. */
int lafs_landmark_theta_bwd(const float* t, const float* dtheta, int B, int n, float* dt, hipStream_t stream);

/* Landmark post-processing (face_pre_pro/ViT_face.py:1347-1378, 698-706): t f32 [B, 2*n_full] raw regressor output ->
 * theta f32 [B, n_out, 2] pixels:  theta = (t - min_b)/(max_b - min_b)*111  (+ noise_scale * noise[B, n_full, 2], the
 * N(0,1)*5 px jitter), landmark k of the output = landmark sel[b,k] of the input (random choice with replacement) or k
 * when sel is NULL. */
int lafs_landmark_theta(const float* t, int B, int n_full, const float* noise, float noise_scale, const int32_t* sel, int n_out,
                        float* theta, hipStream_t stream);
/* Landmark patch gather (face_pre_pro/ViT_face.py:1615-1656): img f32 [B,3,S,S], theta f32 [B,n,2] (x,y pixels) ->
 * mosaic f32 [B,3,8r,8r], r = sqrt(n). */
int lafs_patch_gather_fwd(const float* img, const float* theta, int B, int S, int n, float* mosaic, hipStream_t stream);
/* dtheta(f32) [B,n,2] from dmosaic; dimg (optional, pre-zeroed) accumulates the image gradient. */
int lafs_patch_gather_bwd(const float* img, const float* theta, const float* dmosaic, int B, int S, int n,
                          float* dtheta, float* dimg, hipStream_t stream);
/* Landmark supervision of the fine-tune step (train_largescale.py:807-812 the frozen stage-1 CNN's `land_label`, :815 `pred_land` =
 * the backbone's own theta, :825-836 loss_land = MSELoss()(land_label / 111, pred_land / 111) and loss += land_loss_control * loss_land,
 * :842-843 / acc_step).  pred, label f32 [B, n, 2] pixels (8-byte aligned); weight: DEVICE pointer to this epoch's land_loss_control,
 * read when the kernel runs (&hyper[LAFS_HP_LAND_W]: one captured graph serves every epoch); grad_scale = 1 / acc_step > 0.
 *   loss_land[0]  = mean((pred - label)^2) / 111^2 over all N = 2 B n values, unweighted (what :914-915 prints)
 *   loss[0]      += weight * grad_scale * loss_land                                             (loss may be NULL)
 *   dtheta[b,k,:] += weight * grad_scale * 2 (pred - label) / (111^2 N)                          (dtheta f32 [B, n, 2] may be NULL)
 * `label` is a constant of the backward.  One workgroup, fixed summation order, no atomics: two launches give the same bits; weight 0
 * adds exact zeros.  Nothing but the three outputs is written. */
int lafs_landmark_mse(const float* pred, const float* label, int B, int n, const float* weight, float grad_scale, float* loss_land,
                      float* loss, float* dtheta, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LAFS_HIP_H */
