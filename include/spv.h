/*
 * spv.h -- C-ABI of libspv_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * Spectre-ViT encoder training step.
 *
 * This is the drop-in boundary below the reference's nn.Module surface.  The
 * reference has no native layer at all: every entry point here replaces a chain of stock ATen ops
 * issued by a reference module, cited per function as  <reference file>:<lines>.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed for the duration of the call (nothing is kept,
 *     nothing is allocated); tensors are dense row-major unless a leading dimension is given;
 *   - `dtype` arguments: SPV_F32 (0) or SPV_BF16 (1); statistics, parameters, gradients of
 *     parameters and all accumulation are fp32 regardless;
 *   - `stream` is the hipStream_t to launch on (the caller's current stream); calls never
 *     synchronise and are hipGraph-capturable;
 *   - return value: 0 = ok, non-zero = error (bad shape / alignment / launch failure); the
 *     message is available from spv_last_error() (thread local).
 */
#ifndef SPV_H
#define SPV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPV_F32 0
#define SPV_BF16 1

#define SPV_ABI_VERSION 1

int spv_version(void);
/* Dispatch census (test aid; no reference counterpart): how many calls each kernel family has served in this process, so a
 * parity test can assert that the shapes it ran really took the fused / strip kernels the benchmark times. */
enum {
    SPV_PATH_GEMM_STRIP = 0,     /* gemm_nt_strip_kernel<MB, 0>: store */
    SPV_PATH_GEMM_STRIP_ACC = 1, /* gemm_nt_strip_kernel<MB, 1>: accumulate */
    SPV_PATH_GEMM_TN = 2,        /* every served spv_gemm_tn / _fold call and every spv_gemm_tn_batch GEMM launch, whichever TN kernel ran */
    SPV_PATH_TAIL_LC = 3,        /* lane-contiguous SpectreLinear tail kernels */
    SPV_PATH_TAIL_UP = 4,        /* spv_spectre_tail_bwd_up */
    SPV_PATH_TAIL_LN = 5,        /* spv_spectre_tail_ln_fwd / _bwd */
    SPV_PATH_FNET_MFMA = 6,      /* fnet_mfma_kernel (bf16, dim 512) */
    SPV_PATH_GATHER_LDS = 7,     /* LDS-staged MHPermutMix gather */
    SPV_PATH_DISTILL_CACHED = 8, /* spv_distill_loss_idx_fwd (the distillation loss against the resident teacher-logit cache): one per launch */
    SPV_PATH_GEMM_TN_WIDE = 9,   /* gemm_tn_wide_kernel / gemm_tn_batch_wide_kernel (256 x 128 tile; M % 256 == 0, N % 128 == 0, and for spv_gemm_tn at
                                  * least 4 slabs and 128 workgroups, unless the tall kernel takes the call) */
    SPV_PATH_GEMM_TN_BATCH = 10, /* gemm_tn_batch_kernel / gemm_tn_batch_wide_kernel: up to eight weight gradients in one launch (spv_gemm_tn_batch) */
    SPV_PATH_GEMM_STRIP_POOL = 11, /* gemm_nt_strip_kernel<*, 2 / 3>: data gradient + pooled-broadcast term (spv_gemm_nt_pool_bwd) */
    SPV_PATH_GEMM_ROWS = 13,     /* gemm_nt_rows_kernel: few-rows NT GEMM, one 32 x 32 tile per workgroup, no split-K (the CLS-only last layer) */
    SPV_PATH_PERMUT_ROW0 = 12,   /* spv_permut_row0_fwd / _bwd: MHPermutMix at token row 0 (the CLS-only last layer) */
    SPV_PATH_SPECTRUM = 14,      /* spv_spectrum_log1p (SpectreBranch feature extractor) */
    SPV_PATH_CONV_FWD = 15,      /* spv_conv3x3_fwd */
    SPV_PATH_CONV_DGRAD = 16,    /* spv_conv3x3_dgrad */
    SPV_PATH_CONV_WGRAD = 17,    /* spv_conv3x3_wgrad */
    SPV_PATH_TOKEN_POOL = 18,    /* spv_token_pool_fwd */
    SPV_PATH_TOKEN_UNPOOL = 19,  /* spv_token_pool_bwd */
    SPV_PATH_ATTN_ROW0_FWD = 20, /* spv_attention_row0_fwd (the attention mixer's CLS-only last layer) */
    SPV_PATH_ATTN_ROW0_BWD = 21, /* spv_attention_row0_bwd */
    SPV_PATH_AUGMENT = 22,       /* spv_augment_u8 / spv_loader_fetch_augment (one workgroup per image) or spv_augment_tiled_u8 / spv_loader_fetch_augment_tiled (output tiles): one per call */
    SPV_PATH_TEACHER_VIEW = 23,  /* spv_teacher_view_u8 (the distillation teacher's 224 view, one workgroup per image and row band) */
    SPV_PATH_ATTN_V1 = 24,       /* spv_attention_fwd / _bwd served by the general kernels (attn_*_kernel): one per call */
    SPV_PATH_ATTN_V2 = 25,       /* ... by the LDS-staged kernels (attn2_*_kernel; head dim 16 / 32 / 64) */
    SPV_PATH_ATTN_V3 = 26,       /* ... by the bf16 MFMA flash kernels (attn3_*_kernel; head dim 32 / 64) */
    SPV_PATH_COUNT = 27
};
long long spv_path_count(int which);
const char* spv_last_error(void);

/* ---- precision plumbing -------------------------------------------------------------------
 * torch.autocast's weight cast (spectre_vit/repl/train.py:219) as one kernel; `transpose` also
 * writes the [cols][rows] copy used by the data-gradient GEMM. */
int spv_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* dst[c][r] = src[map(r)][c]; dst leading dimension ld >= rows (pad zero filled).  rows_per_group > 0 reads the
 * grouped source row (r / rows_per_group) * group_stride + row_offset + r % rows_per_group (e.g. the token rows
 * of every image without its CLS row). */
int spv_cast_transpose(const void* src, int src_dtype, void* dst, int dst_dtype, int rows, int cols, int ld,
                       int rows_per_group, int group_stride, int row_offset, void* stream);
/* spv_weight_shadows: both operand layouts of an fp32 nn.Linear weight [rows, cols] (layers.py:85-86) in one pass: the plain
 * copy in the compute dtype (plain may be NULL: fp32 reads the parameter itself) and the transposed copy [cols, ld >= rows]
 * for the data-gradient GEMM.  Rebuilt every training step: optimizers update parameters in place. */
int spv_weight_shadows(const float* w, void* plain, void* transposed, int rows, int cols, int ld, int dtype, void* stream);
/* The same for every weight of a model in one launch: `table` = device array of {const float* src; void* plain; void* transposed;
 * int rows, cols, ld, pad;}; workgroup b serves the 32 x 64 tile (tile_x[b], tile_y[b]) of tensor tile_tensor[b]. */
int spv_weight_shadows_multi(const void* table, const int* tile_tensor, const int* tile_x, const int* tile_y, int ntiles, int dtype,
                             void* stream);

/* ---- dense contraction: C[M,N] = A[M,K] . B[N,K]^T (+ bias[N]) (+ C) ------------------------
 * nn.Linear inside SpectreLinear (spectre_vit/models/spectre/layers.py:85-86,100), its data and
 * weight gradients, and the patch projection (spectre.py:148).  MFMA: v_mfma_f32_32x32x16_bf16
 * (bf16 in) or v_mfma_f32_32x32x2_f32 (exact fp32 in); fp32 accumulate.
 * K, lda, ldb must be multiples of 16 bytes / sizeof(in element); A,B 16-byte aligned.  C and bias take any alignment of their
 * element type (off 16 bytes they are served by element-wide stores and loads); ldc >= N is free.
 * splits > 1: split-K over `splits` slices, fp32 partial slabs in `workspace`
 * (>= splits*M*N*4 bytes, 16-byte aligned), reduced by a second kernel (deterministic).  The slices are whole K-tiles (64 bf16 /
 * 32 fp32 elements), so fewer than `splits` slabs may be written and a request may collapse to one (no workspace access then).
 * Which kernel serves a call: csrc/spv_gemm_core.h (gemm_nt_plan), DESIGN.md "Which GEMM kernel serves a call". */
int spv_gemm_nt(const void* A, const void* B, const float* bias, void* C, int M, int N, int K, int lda,
                int ldb, int ldc, int in_dtype, int out_dtype, int accumulate, int splits,
                void* workspace, void* stream);
/* Same contraction, output row m written to row (m / rows_per_group) * group_stride + row_offset + m % rows_per_group
 * and bias2d[m % rows_per_group][N] added: the patch projection writing straight into the token tensor
 * (position embedding + bias as bias2d, every image's CLS row skipped) -- spectre.py:148-152. */
int spv_gemm_nt_grouped_rows(const void* A, const void* B, const float* bias, const float* bias2d, void* C, int M,
                             int N, int K, int lda, int ldb, int ldc, int in_dtype, int out_dtype,
                             int rows_per_group, int group_stride, int row_offset, void* stream);
/* The same with the dropout that follows the projection (spectre.py:156) applied in the epilogue: the mask of spv_dropout /
 * spv_embed_bwd for the same seed over the flat index of the (contiguous, ldc == N) output: mask(i) = hash(key(i >> 12), i & 4095) for
 * every element, whatever N is (spv_embed_bwd itself needs N % 8 == 0). */
int spv_gemm_nt_grouped_rows_drop(const void* A, const void* B, const float* bias, const float* bias2d, void* C, int M, int N, int K,
                                  int lda, int ldb, int ldc, int in_dtype, int out_dtype, int rows_per_group, int group_stride,
                                  int row_offset, float p_drop, uint64_t seed, void* stream);

/* Data gradient of a SpectreLinear whose skip pools exact windows (in = pool_window * out, the MHPermutMix linear,
 * layers.py:66,93): C[M,N] = A[M,K] . B[N,K]^T + dout[M, N/pool_window][.., n / pool_window] / pool_window -- the
 * transposed average pooling is added in the epilogue instead of going through a rows x N buffer. */
int spv_gemm_nt_pool_bwd(const void* A, const void* B, void* C, const void* dout, int pool_window, int M, int N, int K,
                         int lda, int ldb, int ldc, int in_dtype, int out_dtype, int dout_dtype, void* stream);

/* Multi-GPU runs: keep n CUs (0..128) free of the one-workgroup-per-CU layer GEMM (it needs a whole CU, so a CU that holds a resident
 * RCCL channel would push its workgroup into a second dispatch round).  spectre_vit.dp.GradReducer sets 16 when world_size > 1; the
 * reference has no counterpart (single device, train.py:41). */
int spv_set_reserved_cus(int n);
/* TN contraction C[M,N] = sum_k A[k][m] B[k][n], A [K,lda>=M], B [K,ldb>=N] row-major bf16: the weight gradient
 * dW = dh^T . x (backward of layers.py:86) straight from the row-major activations (transposing LDS reads,
 * ds_read_b64_tr_b16); M, N, lda, ldb multiples of 8; split-K as above, in slices of whole 64-row K-tiles.  K itself is free (a
 * partial last K-tile is zero-filled). */
int spv_gemm_tn(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int out_dtype,
                int accumulate, int splits, void* workspace, void* stream);
/* The same, with up to sixteen folds of row kernels' per-workgroup partial column sums riding in the split-K reduce launch as extra
 * workgroups: out[p][c] = sum_w partials[w][p][c], p < nsum <= 5 (dgamma, dbeta, dbias[, dgamma2, dbeta2]), c < n, fixed order.
 * The row kernel (spv_spectre_tail_bwd*, spv_spectre_tail_ln_bwd, spv_fnet_ln_bwd) is then called with its parameter-gradient
 * pointers NULL: it writes the partials and launches no fold (parts = spv_tail_bwd_parts(rows) for the tails, batch for the FNet
 * kernel).  With one slab (splits == 1, or a request that collapses to one) the folds run as one launch of their own.  The fold jobs
 * are checked before anything is launched: a bad one leaves C untouched.  Why: a 5-us launch between two large kernels costs the
 * step ~20 us (eight per-layer fold launches removed: 157 us of 2.26 ms). */
typedef struct spv_fold_job {
    const float* partials;
    float* out[5];
    int parts, nsum, n;
} spv_fold_job;
int spv_tail_bwd_parts(int rows);
/* Folds with no reduce to ride in: up to any number of jobs in one launch per sixteen (the end-of-backward flush of folds that were
 * held back for a later spv_gemm_tn_fold which never came; sixteen per launch). */
int spv_fold_multi(const spv_fold_job* folds, int nfolds, void* stream);
int spv_gemm_tn_fold(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int out_dtype,
                     int accumulate, int splits, void* workspace, const spv_fold_job* folds, int nfolds, void* stream);
/* Up to 8 weight gradients with the same K (C_i [m_i, n_i] fp32 = A_i[K, lda_i]^T . B_i[K, ldb_i], bf16 operands) in ONE launch
 * + ONE split-K reduce that also carries up to 16 fold jobs.  workspace: splits * sum(m_i * n_i) floats, 16-byte aligned (only the
 * long problems' slabs are written).  m, n, lda, ldb multiples of 8; ldc >= n, a multiple of 4 for a short problem.  For gradients that
 * nobody reads before the backward pass is over (spectre_vit/hip_ops.py holds them back; reference: the nn.Linear weight
 * gradients autograd computes node by node, layers.py:85-101). */
typedef struct spv_tn_problem {
    const void* a;
    const void* b;
    void* c;
    int m, n, lda, ldb, ldc;
    int k;   /* rows THIS problem reduces over: 0 or K = the call's K (split-K as asked); 1..K-1 = a short problem (the CLS-only last
              * layer's 512-row gradients beside the 33 280-row ones): its first k rows, unsplit, stored by the GEMM launch itself */
} spv_tn_problem;
int spv_gemm_tn_batch(const spv_tn_problem* probs, int nprob, int K, int splits, void* workspace, const spv_fold_job* folds, int nfolds,
                      void* stream);
/* The same call as two: part = 1 launches the batched GEMM only, part = 2 the split-K reduce + folds only (same arguments both
 * times).  For a measuring caller that brackets each launch with its own pair of HIP events (bench.py's roofline pass). */
int spv_gemm_tn_batch_part(const spv_tn_problem* probs, int nprob, int K, int splits, void* workspace, const spv_fold_job* folds,
                           int nfolds, int part, void* stream);

/* ---- SpectreLinear tail: out = dropout(GELU_erf(LayerNorm(h)) + adaptive_avg_pool(x)) ---------
 * spectre_vit/models/spectre/layers.py:85-101 (LN eps 1e-5, nn.GELU exact, AdaptiveAvgPool1d over the
 * channel axis; identity skip when k_in == n) + the nn.Dropout that follows it in
 * spectre.py:70-73.  h: [rows,n] pre-norm linear output, x: [rows,k_in] the layer input.
 * Saves mean/rstd [rows] fp32 for the backward.  p_drop == 0 disables dropout. */
int spv_spectre_tail_fwd(const void* h, const void* x, const float* gamma, const float* beta, void* out,
                         float* mean, float* rstd, int rows, int n, int k_in, int dtype, int out_dtype,
                         float p_drop, uint64_t seed, void* stream);

/* Backward of the tail.  dout [rows,n] (dout_dtype) -> dh [rows,n] (dtype), dx_pool [rows,k_in] (dtype; the
 * transposed pooling of the masked dout, to which the caller accumulates dh.W), and the fp32
 * column sums dgamma/dbeta/dbias [n].  `partials` is fp32 scratch of spv_rowop_partial_floats(n)
 * floats.  `dx_add` (nullable, [rows,k_in], dtype): a residual-stream gradient folded into dx_pool
 * (x1 feeds both norm2's residual and linear1, spectre.py:67,70-73), instead of a separate add pass.
 * dx_pool == NULL (the skip gradient is not formed; dx_add is then ignored) is accepted where a kernel honours it: n = 512 (any
 * k_in), n = 3072 from k_in = 768 with h, dout, dh, gamma, beta and partials 16-byte aligned, and k_in a proper multiple of n
 * (exact windows); spv_spectre_tail_bwd_up and spv_spectre_tail_ln_bwd accept it as well.  Every other shape is refused on the host.
 * Rows with n % 4 != 0 (n <= 1024) are served by scalar kernels; their forward stages x in LDS 16 bytes at a time only when both
 * k_in and 2 n are multiples of 4 (the stage starts 2 n floats into LDS), one float at a time otherwise. */
int spv_spectre_tail_bwd(const void* dout, const void* h, const float* mean, const float* rstd,
                         const float* gamma, const float* beta, void* dh, void* dx_pool, float* dgamma,
                         float* dbeta, float* dbias, float* partials, int rows, int n, int k_in, int dtype,
                         int dout_dtype, float p_drop, uint64_t seed, const void* dx_add, void* stream);
int64_t spv_rowop_partial_floats(int n);
/* spv_spectre_tail_bwd for the 512 -> 768 layer (linear1 of the encoder layer, layers.py:85-101 under spectre.py:70-73) that ALSO
 * takes the skip gradient of the layer above (linear3, 768 -> 512) at its source: dout_eff = dout + AdaptiveAvgPool1d^T(mask_up * up_src),
 * up_src [rows, 512] = the gradient that entered linear3's tail (`ds` of spv_spectre_tail_ln_bwd), up_p_drop / up_seed = linear3's
 * dropout.  linear3's backward is then called with dx_pool = NULL and its data-gradient GEMM stores instead of accumulating.
 * spv_tail_up_supported: 1 for (n, k_in) = (768, 512). */
int spv_tail_up_supported(int n, int k_in, int dtype);
int spv_spectre_tail_bwd_up(const void* dout, const void* h, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, void* dh, void* dx_pool, float* dgamma, float* dbeta, float* dbias, float* partials,
                            int rows, int n, int k_in, int dtype, int dout_dtype, float p_drop, uint64_t seed, const void* dx_add,
                            const void* up_src, float up_p_drop, uint64_t up_seed, void* stream);
/* Second half of the encoder layer's elementwise work as ONE kernel each way:
 *   f3 = SpectreLinear3-tail(h3, f1) (as spv_spectre_tail_fwd), x2 = LayerNorm2(x1 + f3)   (spectre.py:67, 70-73)
 * spv_tail_ln_supported: shapes covered (512 outputs from 768 inputs, either dtype); otherwise compose
 * spv_spectre_tail_* with spv_add_layernorm_* (mode 1).
 *   fwd: out = f3 (kept: the backward re-forms x1 + f3 from it), out2 = x2, mean/rstd of the tail's LayerNorm,
 *        mean2/rstd2 of LayerNorm-2; res = x1.
 *   bwd: ds = LayerNorm2-backward(dout2) (written: the residual branch needs it) is used at once as the tail's incoming
 *        gradient; dh, dx_pool (NULL: not formed, see spv_spectre_tail_bwd_up), dgamma, dbeta, dbias as spv_spectre_tail_bwd; dgamma2,
 *        dbeta2 of LayerNorm-2;
 *        partials: spv_tail_ln_partial_floats(n) floats. */
int spv_tail_ln_supported(int n, int k_in, int dtype);
int64_t spv_tail_ln_partial_floats(int n);
int spv_spectre_tail_ln_fwd(const void* h, const void* x, const float* gamma, const float* beta, void* out, float* mean, float* rstd,
                            const void* res, const float* gamma2, const float* beta2, void* out2, float* mean2, float* rstd2, int rows,
                            int n, int k_in, int dtype, float p_drop, uint64_t seed, void* stream);
int spv_spectre_tail_ln_bwd(const void* dout2, const void* f3, const void* res, const float* mean2, const float* rstd2,
                            const float* gamma2, void* ds, float* dgamma2, float* dbeta2, const void* h, const float* mean,
                            const float* rstd, const float* gamma, const float* beta, void* dh, void* dx_pool, float* dgamma,
                            float* dbeta, float* dbias, float* partials, int rows, int n, int k_in, int dtype, float p_drop,
                            uint64_t seed, void* stream);

/* ---- residual + LayerNorm ------------------------------------------------------------------------
 * mode 0: out = LN(a) + b      norm1(mix(x)) + x   spectre_vit/models/spectre/spectre.py:66
 * mode 1: out = LN(a + b)      norm2(x + ff(x))    spectre.py:67
 * backward returns d(LN input) in `din` and dgamma/dbeta; the residual gradient of mode 0's `b`
 * is dout itself. */
/* One-level Haar DWT along the embedding axis + LayerNorm-1 + residual as one row kernel each way (bf16, dim 512 or 1024):
 * out = LN(haar(x)) * gamma + beta + x -- SpectreEncoderLayer's norm1(mix(x)) + x (spectre.py:66) with the 'dwt_embed' mixer of
 * BASELINE config 3 (repl/dwt_experiments.py:56).  Same values as spv_haar_dwt followed by spv_add_layernorm_fwd(mode 0), the bf16
 * rounding of the band tensor between them included; the backward recomputes haar(x) from x, nothing of the mixer is stored.
 * dgamma == NULL: the caller folds `partials` (parts = spv_tail_bwd_parts(rows), nsum = 2, n = dim). */
int spv_haar_ln_supported(int dim, int dtype);
int spv_haar_ln_fwd(const void* x, const float* gamma, const float* beta, void* out, float* mean, float* rstd, int rows, int dim,
                    int dtype, void* stream);
int spv_haar_ln_bwd(const void* dout, const void* x, const float* mean, const float* rstd, const float* gamma, void* dx,
                    float* dgamma, float* dbeta, float* partials, int rows, int dim, int dtype, void* stream);
int spv_add_layernorm_fwd(const void* a, const void* b, const float* gamma, const float* beta, void* out,
                          float* mean, float* rstd, int rows, int n, int mode, int dtype, void* stream);
int spv_add_layernorm_bwd(const void* dout, const void* a, const void* b, const float* mean,
                          const float* rstd, const float* gamma, void* din, float* dgamma, float* dbeta,
                          float* partials, int rows, int n, int mode, int dtype, void* stream);

/* ---- MHPermutMix gather: g[b,f] = x[b, perm[f]] * sign[f], f in [0, heads*d) ------------------------
 * spectre_vit/models/spectre/layers.py:68-72 (advanced-index gather, sign multiply, raw reshape to
 * (B, tokens, embed*heads) -- the reshape is free: g is written flat).  `idx` is the packed table
 * from spv_permut_pack: bit31 = sign (1 => -1), bits 0..30 = source index.
 * backward: dx[b,i] = sum_h sign[h,inv_h(i)] * dg[b,h,inv_h(i)] (each perms[h] is a permutation:
 * no atomics, head by head in LDS). */
/* idx: spv_permut_table_words(heads, d) uint32 words, opaque to the caller: the wide tables uint32 [2][heads][d] -- [0] forward
 * (perm | sign), [1] inverse (inverse perm | sign) -- followed, when d <= 65 536 and d % 8 == 0, by their compact form (uint16
 * indices + one sign bit per element) which the bf16 kernels read instead: every workgroup walks the whole table, so its
 * width is L2 traffic; and, when a bf16 row of d elements does not fit the LDS (Spectre-ViT-Base at 224 / 16), by two sets
 * of scatter lists (backward and forward): per (head, quarter of the output row) the sources whose target lies in that quarter, in
 * ascending order. */
int64_t spv_permut_table_words(int heads, int d);
/* 1 when spv_permut_gather_fwd emits `pooled` for this window on rows longer than the LDS: bf16, d % 8 == 0, heads <= 65 535, and a
 * window that divides d and a quarter of it.  A SHAPE-ONLY answer: the forward refuses what it cannot tell (x or g off 16-byte
 * alignment, batch > 65 535) rather than return with `pooled` unwritten.  Rows that fit the LDS pool by the rule below. */
int spv_permut_pool_supported(int heads, int d, int pool_window, int dtype);
int spv_permut_pack(const int64_t* perms, const float* signs, uint32_t* idx, int heads, int d, void* stream);
/* pooled (nullable, [batch, heads*d / pool_window]): the average of every pool_window consecutive gathered elements
 * (what the SpectreLinear skip needs), produced on the fly so the tail kernel does not re-read g.  A call that is given `pooled`
 * writes all of it or fails:
 *   - a row that fits the LDS (d * elsize <= 150 KiB) in whole 16-byte pieces: window 4, 8, 16 or 32 that divides heads * d, with
 *     (heads * d / 4) % 1024 == 0; anything else is refused ("needs the LDS path" / "unsupported pool window");
 *   - a longer bf16 row: what spv_permut_pool_supported answers;
 *   - x, g and idx 16-byte aligned, else refused.
 * Without `pooled` every shape and every alignment of the element type is served: the kernels that move 16-byte pieces (csrc/
 * spv_permut_core.h names the kernel of every call) need x, g and idx 16-byte aligned; a call that does not meet that runs the
 * element-wide global kernel, which is several times slower. */
int spv_permut_gather_fwd(const void* x, const uint32_t* idx, void* g, void* pooled, int pool_window, int batch,
                          int heads, int d, int dtype, void* stream);
/* Every shape and every alignment of the element type is served; the fast kernels need dg, dx and idx 16-byte aligned (the long-row
 * scatter reads dg one element at a time and needs only dx), otherwise the element-wide global kernel runs. */
int spv_permut_gather_bwd(const void* dg, const uint32_t* idx, void* dx, int batch, int heads, int d,
                          int dtype, void* stream);
/* Token row 0 of the gathered matrix only (the last layer of a stack whose consumer reads the CLS row): g0[b][c] = +-x[b][idx[c]]
 * for the first n = heads * embed entries of the forward table (reference layers.py:71-72: row t of the raw view is the chunk
 * [t n, (t + 1) n) of the flattened (heads, d) gather), x0[b] = the sample's own row 0.  Backward: dx[b] = dx0[b] in row 0, zero
 * elsewhere, + the n scattered values.  idx: the table of spv_permut_pack (its forward part comes first).
 * 0 < n <= d and 0 < embed <= d, else refused (n < embed is fine: all of x0 is written); the backward also refuses d or embed that
 * is not a multiple of 8.  The LDS kernels need x and x0 (dx and dx0) 16-byte aligned, a row of at most 150 KiB and, forward, d and
 * embed multiples of the 16-byte vector; otherwise element-wide kernels in global memory serve the call. */
int spv_permut_row0_fwd(const void* x, const uint32_t* idx, void* g0, void* x0, int batch, int d, int n, int embed, int dtype,
                        void* stream);
int spv_permut_row0_bwd(const void* dg0, const void* dx0, const uint32_t* idx, void* dx, int batch, int d, int n, int embed,
                        int dtype, void* stream);


/* ---- FNet token mixer y = Re(fft2(x)) over (tokens, dim), un-normalised ------------------------------
 * spectre_vit/models/spectre_branch/spectre_branch.py:79, repl/orthogonal_permut.py:23-28 ('fft_bare',
 * spectre.py:31).  The operator is symmetric, so the same call is its own backward.
 * `twiddle`: token-axis cos/sin table of spv_fnet_twiddle_floats(tokens) floats filled once by
 * spv_fnet_make_twiddle (the caller caches it).  `workspace`: fp32 scratch of
 * spv_fnet_workspace_floats(batch,tokens,dim) floats (0 on the LDS fast path: dim a power of two in 8..4096,
 * tokens <= 79 and (tokens+3)*dim*4 <= 160 KiB).  `add_in` (nullable, same shape/dtype as y) is added to the
 * output: in the backward, the residual-stream gradient that bypasses the mixer (spectre.py:66).
 * Alignment: the LDS fast path and the bf16 dim-512 MFMA path (2 <= tokens <= 65) move 16 bytes per access, so x, y and add_in
 * must be 16-byte aligned there; a misaligned pointer is refused on the host.  The two-stage generic path (every shape with a
 * non-zero spv_fnet_workspace_floats) takes any alignment of the element type.  The same holds for x / prenorm / out and
 * dout / prenorm / dx of spv_fnet_ln_*, and for x / out of spv_fnet_cls_fwd and dx of spv_fnet_cls_bwd (16-byte row accesses);
 * gamma and beta are read four floats at a time and must come from 16-byte aligned allocations as well. */
int spv_fnet_mix(const void* x, void* y, const void* add_in, const float* twiddle, int batch, int tokens, int dim,
                 int dtype, float* workspace, void* stream);
int64_t spv_fnet_workspace_floats(int batch, int tokens, int dim);
/* First half of the encoder layer as ONE kernel each way: x1 = LayerNorm1(Re(fft2(x))) + x
 * (spectre_vit/models/spectre/spectre.py:66 with the FFT mixer).  spv_fnet_ln_supported tells whether the fused kernels
 * cover a shape (bf16, dim 512, 2 <= tokens <= 65); otherwise callers compose spv_fnet_mix with spv_add_layernorm_*.
 *   fwd: prenorm = Re(fft2(x)) (kept for the backward), out = LN(prenorm) * gamma + beta + x, mean / rstd [batch*tokens].
 *   bwd: dx = Re(fft2(LN1-backward(dout))) + dout; dgamma / dbeta [dim]; partials: batch * 2 * dim floats of scratch. */
int spv_fnet_ln_supported(int tokens, int dim, int dtype);
int spv_fnet_ln_fwd(const void* x, void* prenorm, void* out, const float* gamma, const float* beta, float* mean, float* rstd,
                    const float* twiddle, int batch, int tokens, int dim, int dtype, void* stream);
int spv_fnet_ln_bwd(const void* dout, const void* prenorm, const float* mean, const float* rstd, const float* gamma, void* dx,
                    float* dgamma, float* dbeta, float* partials, const float* twiddle, int batch, int tokens, int dim, int dtype,
                    void* stream);

/* Row 0 only of the same node, x1[:, 0, :] = LayerNorm1(Re(fft2(x))[0, :]) + x[:, 0, :] -- the last layer of a stack whose
 * consumer reads the CLS row (reference spectre.py:66 + 198).  Token frequency 0 is the sum over tokens: one pass over the sample
 * and ONE dim-point FFT.  out [batch, dim] (dtype), m0 [batch, dim] fp32 (the pre-norm row, kept for the backward), mean / rstd
 * [batch].  Backward: g1 [batch, dim] -> dx [batch, tokens, dim] (every row the same spectrum, row 0 + g1), partials
 * [batch][2][dim] = each sample's dgamma / dbeta contribution (summed by a fold job: spv_fold_multi / a riding fold). */
int spv_fnet_cls_supported(int tokens, int dim, int dtype);
int spv_fnet_cls_fwd(const void* x, const float* gamma, const float* beta, void* out, float* m0, float* mean, float* rstd, int batch,
                     int tokens, int dim, int dtype, void* stream);
int spv_fnet_cls_bwd(const void* g1, const float* m0, const float* mean, const float* rstd, const float* gamma, void* dx,
                     float* partials, int batch, int tokens, int dim, int dtype, void* stream);
int64_t spv_fnet_twiddle_floats(int tokens);
int spv_fnet_make_twiddle(float* twiddle, int tokens, void* stream);

/* FFT module: y[..,k] = sum_d x[..,d] cos(2 pi k d / D), k in [0, D/2]  (rfft(x).real)
 * spectre_vit/modules/spectre.py:9-14.  transpose=1 computes the adjoint (the backward). */
int spv_rfft_real(const void* x, void* y, int rows, int dim, int transpose, int dtype, void* stream);

/* ---- Haar DWT mixers ('dwt_embed' along dim, 'dwt_token' along tokens) ---------------------------
 * named in spectre_vit/models/spectre/spectre.py:33-34; only call site repl/dwt_experiments.py:56.
 * Pairs a=(x0+x1)/sqrt2, d=(x0-x1)/sqrt2 (PyWavelets' 'haar'), output [a_J | d_J | ... | d_1] (pywt.wavedec's order).  `inverse`
 * bit 0: apply the adjoint (the backward; = the inverse when the map is orthonormal).  bit 1 selects what happens to the unpaired
 * last element of an odd length: 0 = it passes through into the approximation band (orthonormal), 1 = pywt's mode="zero" of the
 * reference's call (dwt_experiments.py:56): paired with a zero, a_last = x_last / sqrt2, the duplicate d_last is not stored. */
int spv_haar_dwt(const void* x, void* y, int batch, int tokens, int dim, int axis, int levels, int inverse,
                 int dtype, void* scratch, void* stream);

/* ---- dropout seeds under HIP-graph replay ----------------------------------------------------------------
 * The dropout masks of spectre.py:70-73 / vit.py:30-38 come from a counter hash of (seed, element); seeds are by-value kernel
 * arguments, frozen when a graph is captured.  spv_set_seed_device_ptr(word) makes every dropout kernel add the 64-bit device
 * word to its seed (NULL restores eager behaviour); spv_seed_advance(word, stream) steps it -- captured once per training step, so
 * every replay draws fresh masks.  No reference counterpart (the reference is eager PyTorch). */
int spv_set_seed_device_ptr(const void* seed_word);
int spv_seed_advance(void* seed_word, void* stream);

/* ---- the step prologue: the small launches that open a graph-replayed training step, as one ----------------------------------------
 * spv_seed_advance, spv_weight_shadows_multi, spv_spectral_fold_bf16 (or spv_spectral_fold: fold_out_bf16 NULL), spv_patchify with
 * transposed = 2 and spv_embed_posbias depend on nothing but the parameters and the image, and on each other not at all: one
 * 256-thread launch whose workgroup ranges are dealt to these roles.  Every role is optional -- a NULL leading pointer or a zero count
 * leaves it out -- and a role's workgroup computes what the same workgroup of the separate launch computes: the same bits.
 * Pointers as in the separate entry points (all device memory); the struct itself is read on the host. */
typedef struct spv_prologue_jobs {
    void* seed_word;                                   /* the dropout seed word (spv_seed_advance); NULL: not stepped */
    const void* shadow_table;                          /* spv_weight_shadows_multi's table and tile lists */
    const int* tile_tensor;
    const int* tile_x;
    const int* tile_y;
    int ntiles, shadow_dtype;
    const float* fold_w;                               /* spv_spectral_fold_bf16: proj_w, freq_h, freq_w -> w_full (+ bf16 copy) */
    const float* fold_fh;
    const float* fold_fw;
    float* fold_out;
    void* fold_out_bf16;
    int fold_embed, fold_chans, fold_patch, pad0;
    const float* patch_img;                            /* spv_patchify(img, out, ..., ld, transposed = 2, dtype) */
    void* patch_out;
    int patch_batch, patch_chans, patch_height, patch_width, patch_size, patch_ld, patch_dtype, pad1;
    const float* pos_pos;                              /* spv_embed_posbias(pos, bias, cls, out, patches, embed) */
    const float* pos_bias;
    const float* pos_cls;
    float* pos_out;
    int pos_patches, pos_embed;
} spv_prologue_jobs;
int spv_step_prologue(const spv_prologue_jobs* jobs, void* stream);

/* ---- AdamW over many tensors in one launch ------------------------------------------------------------
 * The optimizer step the script drives: torch.optim.AdamW(lr, betas, weight_decay), spectre_vit/repl/train.py:199-201,237
 * (decoupled weight decay, bias correction; amsgrad / maximize off).  `table`: device array of {float* p; const float* g;
 * float* m; float* v;} per tensor; `sizes[t]` its element count; workgroup c updates elements [chunk_off[c], chunk_off[c] + 2048)
 * of tensor chunk_tensor[c].  one_minus_beta1/2: 1 - beta rounded from double by the caller (torch forms them in double: 1 - 0.999
 * taken in fp32 is off by 1.3e-5).  bias_correction1/2 = 1 - beta^step computed by the caller, or -- step_dev != NULL, for HIP-graph
 * capture -- taken from the device-side step count *step_dev (already advanced for this step). */
int spv_adamw_multi(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                    float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                    float bias_correction1, float bias_correction2, const float* step_dev, void* stream);

/* spv_adamw_multi plus an exponential moving average (EMA) of the weights, updated in the same thread from the registers that hold
 * the new weight p' -- one more 4-byte read and write per element, no extra launch.  p, g, m, v and the step count come out bit for
 * bit as from spv_adamw_multi.  ema_table: DEVICE array of one float* per tensor of `table` (the fp32 EMA buffer, shaped like p; a
 * NULL entry: that tensor is not averaged).  Per averaged element
 *     e' = fmaf(w_t, p' - e, e)          (the difference rounded to fp32, then one fused multiply-add: torch's e.lerp_(p', w_t))
 *     w_t = ema_weight                                          ema_warmup == 0
 *     w_t = max(ema_weight, 9.0f / (10.0f + s))                 ema_warmup != 0  (timm ModelEmaV2: decay = min(d, (1 + n) / (10 + n)))
 * ema_weight = 1 - decay, formed in double and rounded once by the caller (as one_minus_beta1/2), in (0, 1].  s = this step's count,
 * 1 on the first step: *step_dev when step_dev != NULL (so a replayed graph follows the warm-up), else ema_step passed by value.
 * The caller initialises e (a copy of p gives e_1 = p_0 + w_1 (p_1 - p_0)).  An EMA buffer that is not 16-byte aligned is read and
 * written element by element; the arithmetic, and so the result, is the same. */
int spv_adamw_multi_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                        float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                        float bias_correction1, float bias_correction2, const float* step_dev, float* const* ema_table, float ema_weight,
                        int ema_warmup, float ema_step, void* stream);

/* ---- on-device step control: LR schedule, gradient clipping, non-finite skip --------------------------------
 * What the reference's loop does on the host around optimizer.step() -- CosineAnnealingLR (spectre_vit/repl/train.py:202-203),
 * GradScaler's dropped step on an inf / NaN gradient (train.py:205,236-238) and the usual torch.nn.utils.clip_grad_norm_ -- decided
 * on the device, so that a HIP-graph replay (kernel arguments frozen at capture) follows the schedule and the gradient.  Three
 * launches per step: spv_grad_sumsq per parameter group, ONE spv_step_control, spv_adamw_multi_ctl per group.
 *
 * The control block: 64 bytes of device memory, 8-byte aligned, written by spv_step_control with plain vector stores and read by
 * spv_adamw_multi_ctl.  sched_step and skipped are the only fields carried from one step to the next (the caller initialises them,
 * 0 for a fresh run). */
typedef struct spv_step_ctl {
    double a, b;        /* this step's rate of a group: lr = (float)(a * base_lr + b), product and sum each rounded to double */
    float clip_coef;    /* the gradient is multiplied by this in registers: min(1, max_norm / (norm + 1e-6)); 1 without clipping */
    int apply;          /* 0: this step is dropped (non-finite gradient): no parameter, moment or Adam step count changes */
    float grad_norm;    /* L2 norm over every gradient of every group, as the last spv_step_control saw it */
    int sched_step;     /* calls of spv_step_control so far = the schedule's t of the NEXT step (advances on dropped steps too) */
    int skipped;        /* dropped steps so far */
    int micro;          /* gradient accumulation (spv_step_control_accum): micro-steps already in the open window; stays 0 without it */
    int reserved[6];
} spv_step_ctl;
#define SPV_CTL_SCHEDULE 1   /* flags of spv_step_control */
#define SPV_CTL_CLIP 2
#define SPV_CTL_SKIP_NONFINITE 4

/* partials[c] = sum of g^2 over chunk c of the spv_adamw_multi chunk table (table / chunk_tensor / chunk_off / sizes / nchunks as
 * there; only the g pointers are read), formed in fp64: the square of an fp32 value never overflows a double, so the sum is
 * non-finite exactly when an element is, and a large finite gradient stays finite.  One workgroup per chunk, a fixed summation
 * order, no atomics. */
int spv_grad_sumsq(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, double* partials,
                   void* stream);

/* One workgroup: folds partials[0 .. npartials) (every group's, in the caller's order) in a fixed order, then one thread fills *ctl
 * for this step and advances ctl->sched_step.  t = ctl->sched_step on entry, W = warmup_steps, T = total_steps:
 *   SPV_CTL_SCHEDULE        t < W:  lr = base * (t + 1) / (W + 1)                 (torch LinearLR(start_factor=1/(W+1), total_iters=W))
 *                           t >= W: lr = eta_min + (base - eta_min) * (1 + cos(pi * min(t - W, T - W) / (T - W))) / 2
 *                           (torch CosineAnnealingLR(T_max=T-W, eta_min) behind SequentialLR(milestones=[W]); past T the rate STAYS
 *                           at eta_min where torch's closed form would rise again); evaluated in fp64.  Without the flag a = 1, b = 0.
 *   SPV_CTL_CLIP            clip_coef = min(1, max_norm / (norm + 1e-6)) as torch.nn.utils.clip_grad_norm_ (a NaN norm gives a NaN
 *                           coefficient, as there); the gradient tensors themselves are NOT rewritten.
 *   SPV_CTL_SKIP_NONFINITE  apply = 0 and skipped += 1 when the sum of squares is not finite.
 * When the step is applied, *step_ptrs[k] += 1 for k < nsteps: the Adam step counts (one float per parameter group) that
 * spv_adamw_multi_ctl reads through step_dev.  step_ptrs is a DEVICE array of device pointers. */
int spv_step_control(const double* partials, int npartials, float* const* step_ptrs, int nsteps, spv_step_ctl* ctl, int flags,
                     int warmup_steps, int total_steps, double eta_min, float max_norm, void* stream);

/* ---- gradient accumulation: k calls of the step per optimizer step, decided on the device --------------------
 * A window is accumulate_steps = k consecutive micro-steps; ctl->micro counts the micro-steps already in the open window.  Per
 * micro-step: spv_grad_accumulate per parameter group, ONE spv_step_control_accum, spv_adamw_multi_ctl[_ema] per group on a table
 * whose g column holds the accumulators.  One captured graph serves every micro-step; every k-th replay applies the optimizer.
 *
 * spv_grad_accumulate: table / chunk_tensor / chunk_off / sizes / nchunks as spv_grad_sumsq (only the g pointers are read);
 * acc_table is a DEVICE array of one float* per table row, each 16-byte aligned with room for the row's size rounded up to 4.
 * With ctl->micro == 0, acc = g: an assignment, the old contents are not read (a NaN left there vanishes).  Otherwise
 * acc = (float)(acc + g), one IEEE add per element.  partials[c] = the fp64 sum of squares of the NEW acc over chunk c, in
 * spv_grad_sumsq's order and arithmetic (with micro == 0 its bits).  g need not be 16-byte aligned.  Plain vector loads and stores. */
int spv_grad_accumulate(const void* table, float* const* acc_table, const int* chunk_tensor, const int* chunk_off, const int* sizes,
                        int nchunks, const spv_step_ctl* ctl, double* partials, void* stream);

/* spv_step_control for a window of accumulate_steps = k >= 1 micro-steps (arguments as there).  m = ctl->micro on entry:
 *   m <  k - 1   apply = 0, micro = m + 1; nothing else in *ctl changes and no Adam step count moves.
 *   m >= k - 1   the boundary: sumsq folded as spv_step_control does, norm = (float)(sqrt(sumsq) / (double)k) -- the norm of the MEAN
 *                gradient, stored as grad_norm; the schedule at t = sched_step, sched_step += 1 (one tick per window, applied or
 *                dropped); c = spv_step_control's clip expression on norm (1 without SPV_CTL_CLIP) and
 *                clip_coef = (float)((double)c / (double)k), so that acc * clip_coef is the clipped mean; apply = 0 and skipped += 1
 *                exactly when SPV_CTL_SKIP_NONFINITE is set and sumsq is not finite (non-finiteness is sticky under addition, so
 *                deciding at the boundary is exact), otherwise apply = 1 and *step_ptrs[i] += 1; micro = 0 either way.
 * With k = 1 every expression reduces bit for bit to spv_step_control's. */
int spv_step_control_accum(const double* partials, int npartials, float* const* step_ptrs, int nsteps, spv_step_ctl* ctl, int flags,
                           int warmup_steps, int total_steps, double eta_min, float max_norm, int accumulate_steps, void* stream);

/* spv_adamw_multi with lr = (float)(ctl->a * base_lr + ctl->b), the gradient scaled by ctl->clip_coef in registers and nothing
 * written at all when ctl->apply == 0.  The same update body as spv_adamw_multi: with a = 1, b = 0, clip_coef = 1, apply = 1 the
 * results are bit for bit its results.  step_dev (required): the group's Adam step count, already advanced by spv_step_control. */
int spv_adamw_multi_ctl(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, double base_lr,
                        float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                        const float* step_dev, const spv_step_ctl* ctl, void* stream);

/* spv_adamw_multi_ctl plus the moving average of spv_adamw_multi_ema (ema_table / ema_weight / ema_warmup as there; s = *step_dev, which
 * spv_step_control advanced).  A dropped step (ctl->apply == 0) writes nothing, the average included. */
int spv_adamw_multi_ctl_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, double base_lr,
                            float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                            const float* step_dev, const spv_step_ctl* ctl, float* const* ema_table, float ema_weight, int ema_warmup,
                            void* stream);

/* ---- torch.optim.Adam and torch.optim.SGD on the same launches ------------------------------------------------
 * The two other optimizer lines of the script (spectre_vit/repl/train.py:197-198, :307).  Chunk tables, control block, step counts
 * and the moving average are AdamW's; the four forms of each rule take the arguments of the spv_adamw_multi form of the same suffix.
 *
 * Adam (amsgrad / maximize off): AdamW's expressions with the decay in the gradient, d = g * clip + weight_decay * p (product and sum
 * rounded separately; nothing added when weight_decay == 0), and no decoupled factor.  With weight_decay == 0 the results equal
 * spv_adamw_multi*'s bit for bit.  Checked besides AdamW's checks: betas in [0, 1), eps >= 0, weight_decay >= 0, lr >= 0. */
int spv_adam_multi(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr, float beta1,
                   float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay, float bias_correction1,
                   float bias_correction2, const float* step_dev, void* stream);
int spv_adam_multi_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                       float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                       float bias_correction1, float bias_correction2, const float* step_dev, float* const* ema_table, float ema_weight,
                       int ema_warmup, float ema_step, void* stream);
int spv_adam_multi_ctl(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, double base_lr,
                       float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                       const float* step_dev, const spv_step_ctl* ctl, void* stream);
int spv_adam_multi_ctl_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, double base_lr,
                           float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                           const float* step_dev, const spv_step_ctl* ctl, float* const* ema_table, float ema_weight, int ema_warmup,
                           void* stream);

/* SGD (maximize off).  `table` rows are {float* p; const float* g; float* buf; unused}; buf is neither read nor written (and may be
 * NULL) with momentum == 0.  Per element, every line ONE fp32 rounding, the same on the float4 and on the scalar walk:
 *     d = g                                   (_ctl: d = g * clip_coef)
 *     weight_decay != 0:   t = weight_decay * p;  d = d + t
 *     momentum != 0:       s == 1:  buf = d       else:  t1 = momentum * buf;  t2 = one_minus_dampening * d;  buf = t1 + t2
 *                          nesterov:  t = momentum * buf;  d = d + t           else:  d = buf
 *     t = lr * d;  p = p - t
 * s = the group's step count of this step, already advanced (1 on its first applied step, where torch clones the gradient into the
 * buffer): *step_dev, or -- step_dev == NULL, spv_sgd_multi[_ema] only -- `step` by value (>= 1).  The _ema forms' warm-up reads the
 * same s.  one_minus_dampening = 1 - dampening formed in double and rounded once by the caller.  Checked: momentum in [0, 1),
 * one_minus_dampening in (0, 1] (dampening in [0, 1)), weight_decay >= 0, lr >= 0, nesterov only with momentum > 0 and dampening == 0. */
int spv_sgd_multi(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr, float momentum,
                  float one_minus_dampening, float weight_decay, int nesterov, float step, const float* step_dev, void* stream);
int spv_sgd_multi_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                      float momentum, float one_minus_dampening, float weight_decay, int nesterov, float step, const float* step_dev,
                      float* const* ema_table, float ema_weight, int ema_warmup, void* stream);
int spv_sgd_multi_ctl(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, double base_lr,
                      float momentum, float one_minus_dampening, float weight_decay, int nesterov, const float* step_dev,
                      const spv_step_ctl* ctl, void* stream);
int spv_sgd_multi_ctl_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, double base_lr,
                          float momentum, float one_minus_dampening, float weight_decay, int nesterov, const float* step_dev,
                          const spv_step_ctl* ctl, float* const* ema_table, float ema_weight, int ema_warmup, void* stream);

/* ---- Walsh-Hadamard butterflies along the last axis -----------------------------------
 * spectre_vit/models/spectre/hadamar.py: fwht :12-32 / hadamard_transform :83-112 (mode 0, natural order; scale = n^-1/2
 * when normalised), fwht_fast :58-80 (mode 1: every stage interleaves sum / difference, un-normalised) and its transpose
 * (mode 2: the backward of mode 1; mode 0 is its own transpose).  LearnableHadamard.forward :127-141 is ONE call: rows of
 * n_in values zero-padded to n (a power of two), `repeat` = num_blocks passes, the first n_out values kept, `residual`
 * (nullable, [rows, n_out]) added.  x [rows, n_in], y [rows, n_out]; n <= 16384. */
int spv_fwht(const void* x, void* y, const void* residual, int rows, int n_in, int n, int n_out, int mode, int repeat,
             float scale, int dtype, void* stream);

/* ---- Walsh-Hadamard token mixer  y = crop_{N,D}( H_Np . pad_{Np,Dp}(x) . H_Dp ) . scale  over (tokens, dim) -------------------
 * The 2-D operator of the same file's functions: fwht(fwht(F.pad(x, (0, Dp - D, 0, Np - N)), dim=-1), dim=-2)[..., :N, :D] with
 * Np / Dp = next_pow2 (hadamar.py:12-32, LearnableHadamard's pad / crop :130-139); H natural order (Sylvester); the caller passes
 * scale = (Np Dp)^-1/2 for fwht's default normalize=True, 1 otherwise.  crop = pad^T and H is symmetric, so the same call is its
 * own backward.  `add_in` (nullable, same shape / dtype as y) is added to the output: in the backward, the residual-stream gradient
 * that bypasses the mixer (spectre.py:66).  fp32 and bf16; any tokens >= 1, any dim >= 1 with Dp <= 16384.
 *   one kernel   dim % 8 == 0, tokens <= 128 and tokens * Dp * 4 <= 160 KiB (the padded image in LDS as fp32, no other scratch): one
 *                read of x, one write of y.  Moves 16 bytes per access: x, y and add_in must be 16-byte aligned, else refused.
 *   generic      everything else with Np <= 32768: rows along dim into `workspace` (spv_hadamard_workspace_floats floats, fp32), then
 *                column slabs along tokens.  Any alignment of the element type.
 * spv_hadamard_path: which of the two spv_hadamard_mix would take for a shape (the answer of the host-pure selector in
 * csrc/spv_hadamard_core.h, which the entry point itself switches on), or why it refuses.  Pointer alignment is not a shape: a
 * misaligned one-kernel call is refused by spv_hadamard_mix itself. */
#define SPV_HADAMARD_ONE_KERNEL 1
#define SPV_HADAMARD_GENERIC 2
#define SPV_HADAMARD_REFUSE_EMPTY (-1)      /* tokens < 1 or dim < 1 */
#define SPV_HADAMARD_REFUSE_DTYPE (-2)
#define SPV_HADAMARD_REFUSE_DIM (-3)        /* next_pow2(dim) > 16384 */
#define SPV_HADAMARD_REFUSE_TOKENS (-4)     /* generic path: next_pow2(tokens) > 32768 */
#define SPV_HADAMARD_REFUSE_WORKSPACE (-5)  /* generic path without a workspace */
int spv_hadamard_path(int dtype, int tokens, int dim, int has_workspace);
int64_t spv_hadamard_workspace_floats(int batch, int tokens, int dim);
int spv_hadamard_mix(const void* x, void* y, const void* add_in, int batch, int tokens, int dim, float scale, int dtype,
                     float* workspace, void* stream);
/* First half of the encoder layer as ONE kernel each way: x1 = LayerNorm1(mix(x)) + x (spectre.py:66 with the Hadamard mixer), the
 * argument shape of spv_fnet_ln_fwd / _bwd with `scale` in the twiddle table's place.  Window (spv_hadamard_ln_supported): bf16,
 * dim 512, 2 <= tokens <= 65; otherwise callers compose spv_hadamard_mix with spv_add_layernorm_*.
 *   fwd: prenorm = mix(x) (kept for the backward), out = LN(prenorm) * gamma + beta + x, mean / rstd [batch * tokens].
 *   bwd: dx = mix(LN1-backward(dout)) + dout; partials: batch * 2 * dim floats = each sample's dgamma / dbeta contribution;
 *        dgamma / dbeta [dim], or both NULL: the caller folds `partials` (parts = batch, nsum = 2, n = dim: spv_fold_multi or a
 *        riding fold).
 * The token axis runs on the MFMA against the +-1 corner H_Np[:N, :N] (exact in bf16); the backward's fp32 LayerNorm gradient enters
 * it as a hi + lo pair of bf16 values.  No global scratch.  x / prenorm / out, dout / dx, gamma and beta 16-byte aligned. */
int spv_hadamard_ln_supported(int tokens, int dim, int dtype);
int spv_hadamard_ln_fwd(const void* x, void* prenorm, void* out, const float* gamma, const float* beta, float* mean, float* rstd,
                        float scale, int batch, int tokens, int dim, int dtype, void* stream);
int spv_hadamard_ln_bwd(const void* dout, const void* prenorm, const float* mean, const float* rstd, const float* gamma, void* dx,
                        float* dgamma, float* dbeta, float* partials, float scale, int batch, int tokens, int dim, int dtype,
                        void* stream);
/* Row 0 only of the same node (the last layer of a stack whose consumer reads the CLS row, as spv_fnet_cls_*): row 0 of H_Np is all
 * ones, so m0 = scale * H_D . (sum over tokens of x): one pass over the sample and ONE dim-point transform.  dim 256 / 512 / 1024,
 * tokens >= 1, both dtypes.  out [batch, dim], m0 [batch, dim] fp32, mean / rstd [batch].  Backward: g1 [batch, dim] -> dx [batch,
 * tokens, dim] (every row the same transformed row, row 0 + g1), partials [batch][2][dim].  x, out and dx 16-byte aligned. */
int spv_hadamard_cls_supported(int tokens, int dim, int dtype);
int spv_hadamard_cls_fwd(const void* x, const float* gamma, const float* beta, void* out, float* m0, float* mean, float* rstd,
                         float scale, int batch, int tokens, int dim, int dtype, void* stream);
int spv_hadamard_cls_bwd(const void* g1, const float* m0, const float* mean, const float* rstd, const float* gamma, void* dx,
                         float* partials, float scale, int batch, int tokens, int dim, int dtype, void* stream);

/* ---- learnable global filter along the token axis --------------------------------------
 * For x (batch, tokens, dim) and K = tokens / 2 + 1:
 *   X = rfft(x, dim=1, norm="ortho");  y = irfft(X * W, n=tokens, dim=1, norm="ortho")
 * W = `filter` read as (K, dim) complex: fp32 (K, dim, 2), real part first.  irfft ignores the imaginary part of the DC bin and, when
 * tokens is even, of the Nyquist bin: the kernels read those entries as 0 and their gradient is exactly +0.  fp32 and bf16 x / y;
 * filter, tables, gradients of the filter and all arithmetic fp32.  Any tokens in 1..2730, any dim >= 1, any element alignment.
 *   fast         bf16, dim % 64 == 0, tokens <= 80: both token-axis products on the MFMA against DFT tables split into hi + lo bf16, the
 *                spectrum on chip as hi + lo bf16; one workgroup per (sample, 64 columns), x read once and y written once in 16-byte
 *                pieces.  x, y (dy, dx) and tables must be 16-byte aligned, else the call is refused.
 *   generic      everything else: one workgroup per (sample, block of up to 64 columns), fp32 direct sums, the spectrum in LDS.  Any
 *                alignment of the element type.
 * spv_gfilter_path: which kernel serves a shape, or why it is refused (the host-pure selector of csrc/spv_gfilter_core.h, which the
 * entry points switch on); `aligned`: the pointers above sit on 16 bytes.
 *   tables     spv_gfilter_table_floats(tokens) floats, filled once per token count by spv_gfilter_make_tables.
 *   workspace  spv_gfilter_workspace_floats floats of fp32 scratch (0 for both paths: NULL is accepted).
 *   bwd        from x and dy alone (X is recomputed): dx = irfft(rfft(dy) * conj(W_eff)) and dfilter [K][dim][2] =
 *              c_k * sum_b conj(X) G, c_k = 1 at the DC / Nyquist bins, else 2.  A workgroup sums over the samples it owns into one of
 *              min(batch, 32) fp32 slabs (`partials`, spv_gfilter_partial_floats floats), folded in the fixed order of every other
 *              fold of the library: no atomics, equal bits from equal inputs. */
#define SPV_GFILTER_FAST 1
#define SPV_GFILTER_GENERIC 2
#define SPV_GFILTER_REFUSE_EMPTY (-1)       /* tokens < 1 or dim < 1 */
#define SPV_GFILTER_REFUSE_DTYPE (-2)       /* neither SPV_F32 nor SPV_BF16 */
#define SPV_GFILTER_REFUSE_ALIGN (-4)       /* a shape of the fast window with a pointer off 16-byte alignment */
#define SPV_GFILTER_REFUSE_TOKENS (-3)      /* tokens > 2730: the table and one column of the backward no longer fit 64 KiB of LDS */
int spv_gfilter_path(int dtype, int tokens, int dim, int aligned);
int64_t spv_gfilter_table_floats(int tokens);
int spv_gfilter_make_tables(float* tables, int tokens, void* stream);
int64_t spv_gfilter_workspace_floats(int batch, int tokens, int dim);
int64_t spv_gfilter_partial_floats(int batch, int tokens, int dim);
int spv_gfilter_fwd(const void* x, const float* filter, void* y, const float* tables, int batch, int tokens, int dim, int dtype,
                    float* workspace, void* stream);
int spv_gfilter_bwd(const void* x, const void* dy, const float* filter, void* dx, float* dfilter, const float* tables, float* partials,
                    int batch, int tokens, int dim, int dtype, float* workspace, void* stream);

/* ---- patch embedding ---------------------------------------------------------------------------
 * tokens[b,0,:] = cls + pos[0]; tokens[b,1+n,:] = W_full . patch(b,n) + bias + pos[1+n]
 * where patch(b,n) is the (c,p,q)-ordered P x P pixel block.  With W_full = conv weight this is
 * PatchEmbedding (spectre_vit/modules/patch_embeddings.py:28-43); with
 * W_full = (proj.weight * freq_h (x) freq_w) . R, R = Re(rfft2 ortho) it is SpectralPatchEmbed
 * (spectre_vit/models/spectre/spectre.py:124-156).  The contraction itself is spv_gemm_nt_grouped_rows;
 * these entry points are the plumbing around it:
 *   spv_patchify        pixel blocks -> [B*Np, ld>=K] rows (transposed = 0), the [K, ld>=B*Np] transpose (1), or token rows
 *                       [B][Np+1][ld>=K] whose first row per image -- the CLS slot -- is zero (2: the token GEMM and the TN
 *                       weight-gradient GEMM read that layout as it lies)
 *   spv_embed_posbias   bias2d[t][e] = pos[1+t][e] + bias[e]; with cls != NULL one more row in front: cls[e] + pos[0][e]
 *                       (out then has patches + 1 rows and the GEMM over the zero CLS rows writes the CLS tokens)
 *   spv_embed_cls_rows  tokens[b,0,:] = cls + pos[0]
 *   spv_spectral_fold / _bwd   W_full from (proj.weight, freq_h, freq_w) and the gradients back
 *                       (scratch: embed*chans*patch*(patch/2+1) floats)
 *   spv_dropout         y = x * mask(seed, index) / (1-p): nn.Dropout (spectre.py:154) with a counter-based
 *                       mask that the backward regenerates (same call on the gradient). */
int spv_patchify(const float* img, void* out, int batch, int chans, int height, int width, int patch, int ld,
                 int transposed, int out_dtype, void* stream);
/* spv_patchify_u8: the same rows from the data loader's uint8 HWC batch [B,H,W,C], normalised on the fly as
 * ToTensor + Normalize(mean, std) do on the host (spectre_vit/repl/train.py:102-112):
 * (pixel / 255 - mean[c]) * inv_std[c]. */
int spv_patchify_u8(const unsigned char* img_hwc, const float* mean, const float* inv_std, void* out, int batch, int chans,
                    int height, int width, int patch, int ld, int transposed, int out_dtype, void* stream);
int spv_embed_posbias(const float* pos, const float* bias, const float* cls, float* out, int patches, int embed, void* stream);
int spv_embed_cls_rows(const float* cls, const float* pos, void* tokens, int batch, int tokens_per_image, int embed,
                       int dtype, void* stream);
int spv_spectral_fold(const float* proj_w, const float* freq_h, const float* freq_w, float* w_full, int embed,
                      int chans, int patch, void* stream);
/* spv_spectral_fold that also writes the bf16 copy the token GEMM reads in a bf16 step (one launch instead of fold + cast) */
int spv_spectral_fold_bf16(const float* proj_w, const float* freq_h, const float* freq_w, float* w_full, void* w_full_bf16, int embed,
                           int chans, int patch, void* stream);
int spv_spectral_fold_bwd(const float* dw_full, const float* proj_w, const float* freq_h, const float* freq_w,
                          float* dproj_w, float* dfreq_h, float* dfreq_w, float* scratch, int embed, int chans,
                          int patch, void* stream);
int spv_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int dtype, void* stream);
/* The token GEMM of the embedding's forward on a kernel of its own (thin K: the 128 x 128 tile kernel ran 1040 tiles of one K step each):
 *   tokens[r][:] = bf16((patches[r][:] . w^T + posbias[r % tokens_per_image][:]) * dropout_scale),  r < rows
 * patches [rows, k] bf16 token rows (spv_patchify, transposed = 2: the zero CLS row of every image makes row 0 of posbias -- cls + pos[0] --
 * land there by itself), w [n, k] bf16, posbias [tokens_per_image, n] fp32 (spv_embed_posbias with cls), tokens [rows, n] bf16,
 * contiguous.  Exactly spv_gemm_nt_grouped_rows_drop(patches, w, NULL, posbias, tokens, rows, n, k, k, k, n, SPV_BF16, SPV_BF16,
 * tokens_per_image, tokens_per_image, 0, p_drop, seed, stream), bit for bit: v_mfma_f32_32x32x16_bf16 over k / 16 steps in ascending k from
 * a zero accumulator with the same operand roles, + the posbias row, * the dropout scale, one rounding to bf16; the mask is that call's
 * (spv_dropout's on the flat index r * n + col with the same seed), so spv_embed_bwd finds it.
 * spv_token_embed_supported: 1 when dtype == SPV_BF16, rows > 0, k % 16 == 0, 16 <= k <= 64 and n % 64 == 0 (n > 0); every other call
 * stays with spv_gemm_nt_grouped_rows_drop.  spv_token_embed_fwd refuses, before any launch, an unsupported shape, tokens_per_image <= 0,
 * p_drop outside [0, 1), a NULL pointer and a pointer off 16-byte alignment. */
int spv_token_embed_supported(int rows, int n, int k, int dtype);
int spv_token_embed_fwd(const void* patches, const void* w, const float* posbias, void* tokens, int rows, int n, int k,
                        int tokens_per_image, float p_drop, uint64_t seed, void* stream);
/* Backward of the token tensor in one pass + one fold: dtok = dropout_mask(g [+ gcls on the CLS rows]) (the mask of the forward's
 * spv_dropout with the same seed over the same flat index; dtok may be NULL when it would equal g), and the sums over the batch that
 * dpos [tokens][embed], dbias[e] = sum_{t >= 1} dpos[t][e] and dcls[e] = dpos[0][e] are (gradients of position_embeddings, proj.bias
 * and cls_token, spectre.py:133-135,150-155).  partials: spv_embed_bwd_groups(batch) * tokens * embed floats. */
int spv_embed_bwd_groups(int batch);
int spv_embed_bwd(const void* g, const void* gcls, void* dtok, float* partials, float* dpos, float* dbias, float* dcls, int batch,
                  int tokens, int embed, float p_drop, uint64_t seed, int dtype, void* stream);

/* ---- softmax attention core for the baseline ViT ------------------------------------------------
 * nn.MultiheadAttention inside the stock nn.TransformerEncoderLayer, spectre_vit/models/vit/vit.py:30-38:
 * ctx = dropout(softmax(Q K^T / sqrt(head_dim))) V per (sequence, head).
 * qkv [seqs, len, 3*heads*head_dim] (q|k|v), ctx/dctx [seqs, len, heads*head_dim], probs and dscores
 * [seqs, heads, len, len] (probs is saved for the backward, dscores is scratch of the same size).
 * len <= 1024, head_dim <= 128.  Which tensor axis is `len` is the caller's business: the reference feeds (B,N,E) with
 * batch_first=False, so len = B. */
int spv_attention_fwd(const void* qkv, void* ctx, void* probs, int seqs, int len, int heads, int head_dim, int dtype,
                      float p_drop, uint64_t seed, void* stream);
int spv_attention_bwd(const void* dctx, const void* qkv, const void* probs, void* dscores, void* dqkv, int seqs, int len,
                      int heads, int head_dim, int dtype, float p_drop, uint64_t seed, void* stream);
/* The same attention for query row 0 only (SpectreViT(mixer="attention"): its last layer's output is read at the CLS row alone):
 * ctx0[b, h] = dropout(softmax(q0[b, h] . K[b, :, h]^T / sqrt(head_dim))) . V[b, :, h], with the dropout mask spv_attention_fwd
 * applies at query row 0 of the same (sample, head) for the same seed.  q0 / ctx0 / dctx0 / dq0 [batch, E] dense (E = heads *
 * head_dim); K, V [batch, len, E] at row stride ldkv elements (a packed [batch, len, 2E] k|v projection: ldkv = 2E); dK, dV at row
 * stride ldd, written densely (every key row); probs [batch, heads, len] fp32 = the softmax before the mask (written by the forward
 * unless NULL, read by the backward).  E a multiple of 8 (bf16) / 4 (fp32) and <= 256 times that, ldkv / ldd likewise, K / V / dK /
 * dV 16-byte aligned, heads * len <= 8192.  Deterministic: every output element has one writer, no atomics. */
int spv_attention_row0_fwd(const void* q0, const void* k, const void* v, int ldkv, void* ctx0, float* probs, int batch, int len,
                           int heads, int head_dim, int dtype, float p_drop, uint64_t seed, void* stream);
int spv_attention_row0_bwd(const void* dctx0, const void* q0, const void* k, const void* v, int ldkv, const float* probs, void* dq0,
                           void* dk, void* dv, int ldd, int batch, int len, int heads, int head_dim, int dtype, float p_drop,
                           uint64_t seed, void* stream);

/* ---- generic helpers used by the module mirror ------------------------------------------------------
 * GELU (TransformerEncoderLayer MLP, vit.py:30-36), column sums (bias / position-embedding gradients;
 * partials: >= min(rows,512)*n floats), a*x + b*y. */
int spv_gelu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream);
int spv_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype, void* stream);
int spv_colsum(const void* x, float* out, float* partials, int rows, int n, int dtype, void* stream);
int spv_axpby(const void* x, const void* y, void* out, float a, float b, int64_t n, int dtype, void* stream);

/* ---- the classifier end of the step: SpectreLinear over a few rows, and mean cross-entropy -------------------------
 * The class head  mlp_head = SpectreLinear(embed, classes)  (spectre_vit/models/spectre/spectre.py:190-192, applied to
 * (x + src)[:, 0] :199-202) and  nn.CrossEntropyLoss()  (spectre_vit/repl/train.py:196,226).  For rows <= 4096,
 * n <= 128, k <= 1024, n <= k (spv_small_sl_supported) the whole SpectreLinear -- x = xa[row*lda] (+ xb[row*ldb]),
 * h = x W^T + b over the fp32 master weights, LayerNorm, exact-erf GELU, adaptive-average-pooled skip -- is ONE
 * launch; its backward two (rows: dh, dx, partial column sums; weights: dW and the fold of dgamma/dbeta/dbias).
 * out, h, xs (the summed input, fp32 [rows,k]), mean, rstd are written by the forward and read by the backward;
 * partials: spv_small_sl_partial_floats(rows, n) floats; dtype = type of xa / xb / dx. */
int spv_small_sl_supported(int rows, int n, int k);
int64_t spv_small_sl_partial_floats(int rows, int n);
int spv_small_sl_fwd(const void* xa, int64_t lda, const void* xb, int64_t ldb, const float* W, const float* bias,
                     const float* gamma, const float* beta, float* out, float* h, float* xs, float* mean, float* rstd,
                     int rows, int n, int k, int dtype, void* stream);
int spv_small_sl_bwd(const float* dout, const float* h, const float* xs, const float* mean, const float* rstd,
                     const float* W, const float* gamma, const float* beta, float* dh, void* dx, float* dW,
                     float* dgamma, float* dbeta, float* dbias, float* partials, int rows, int n, int k, int dx_dtype,
                     void* stream);
/* The two launches of spv_small_sl_bwd on their own (it calls both, in this order).  Nothing inside a backward pass reads dW, dgamma,
 * dbeta or dbias, so a caller may issue the weights launch later, beside other work: it reads dh and partials (written by the rows
 * launch) and xs, in 256-thread workgroups with 4 KB of LDS.  Same bits either way. */
int spv_small_sl_bwd_rows(const float* dout, const float* h, const float* mean, const float* rstd, const float* W,
                          const float* gamma, const float* beta, float* dh, void* dx, float* partials, int rows, int n, int k,
                          int dx_dtype, void* stream);
int spv_small_sl_bwd_w(const float* dh, const float* xs, const float* partials, float* dW, float* dgamma, float* dbeta,
                       float* dbias, int rows, int n, int k, void* stream);
/* loss = mean_r(logsumexp(logits[r]) - logits[r][labels[r]]) (fp32 logits [rows, classes], int64 labels; a label outside
 * [0, classes) makes the loss NaN).  lse [rows] is kept for the backward: dlogits = (softmax - onehot) * grad_out[0] / rows.
 * workspace: spv_cross_entropy_workspace_floats() floats, ZEROED ONCE by the caller (it holds an arrival counter that
 * every launch re-arms); the sum over rows is taken in a fixed order. */
int64_t spv_cross_entropy_workspace_floats(void);
int spv_cross_entropy_fwd(const float* logits, const int64_t* labels, float* lse, float* loss, float* workspace, int rows,
                          int classes, void* stream);
int spv_cross_entropy_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_out,
                          float* dlogits, int rows, int classes, void* stream);

/* ---- SpectreBranch feature extractor (spectre_vit/models/spectre_branch/spectre_branch.py:122-173) ----------------------------
 * Stage maps are channels-last (B, H, W, C), dense.  The 3x3 convolution (valid, stride 1, spectre_branch.py:133) is an im2col GEMM
 * on spv_gemm_nt with K ordered (c, ky, kx), the order of the PyTorch weight [Cout][Cin][3][3]; Kp = 9 Cin rounded up to 8.
 *
 * spv_spectrum_log1p: out[b][u][v][c] = log1p(|rfft2(img[b][c])[u][v]|), v < W/2 + 1 (spectre_branch.py:151); img fp32 NCHW, out in
 * `dtype`.  One workgroup per plane, the plane's row transform in LDS: spv_spectrum_floats(H, W) floats, at most 16384. */
int spv_spectrum_floats(int H, int W);
int spv_spectrum_log1p(const float* img, void* out, int B, int C, int H, int W, int dtype, void* stream);
/* y[(b,ho,wo)][co] = bias[co] + sum_k cols[(b,ho,wo)][k] w[co][k]: w [Cout][Kp] (zero past 9 Cin), cols a workspace of
 * B (H-2) (W-2) Kp elements of `dtype`, y [B (H-2) (W-2)][Cout] in `dtype`. */
int spv_conv3x3_fwd(const void* x, const void* w, const float* bias, void* y, void* cols, int B, int H, int W, int Cin, int Cout,
                    int dtype, void* stream);
/* dx [B H W][Cin] = the full correlation of dy [B (H-2) (W-2)][Cout] with the kernel: wd [Cin][Kd], wd[c][(co, ky, kx)] = w[co][c][ky][kx],
 * Kd = 9 Cout rounded up to 8 (zero past 9 Cout); cols a workspace of B H W Kd elements. */
int spv_conv3x3_dgrad(const void* dy, const void* wd, void* dx, void* cols, int B, int H, int W, int Cin, int Cout, int dtype,
                      void* stream);
/* dw [Cout][9 Cin] fp32 (the parameter's layout) = dy^T . im2col(x), a reduction over the M = B (H-2) (W-2) positions, split in
 * `splits` K-slices (workspace >= splits Cout 9 Cin floats) and folded in a fixed order.  Workspaces: dyt Cout Mp and colst 9 Cin Mp
 * elements of `dtype`, Mp = M rounded up to 8.  The bias gradient is spv_colsum of dy. */
int spv_conv3x3_wgrad(const void* dy, const void* x, float* dw, void* dyt, void* colst, float* workspace, int splits, int B, int H,
                      int W, int Cin, int Cout, int dtype, void* stream);
/* AdaptiveAvgPool1d(T) over the flattened H W = L positions of y [B][L][C] (spectre_branch.py:144), token-major: out [B][T][ldo],
 * window t = [floor(t L / T), ceil((t + 1) L / T)), columns C..ldo-1 written zero.  L < T is allowed (windows overlap). */
int spv_token_pool_fwd(const void* y, void* out, int B, int L, int C, int T, int ldo, int dtype, void* stream);
/* its transpose: dy [B][L][C] = sum over the windows holding l of dout[b][t][c] / |window t| (+ add [B][L][C] when not NULL) */
int spv_token_pool_bwd(const void* dout, int ldo, const void* add, void* dy, int B, int L, int C, int T, int dtype, void* stream);

/* ---- training augmentation: the transform chain of spectre_vit/repl/train.py:100-115 on the device --------------------------
 * RandomHorizontalFlip -> ColorJitter -> RandomGrayscale -> RandomAffine(degrees) -> RandomApply([GaussianBlur(3)]) -> ToTensor ->
 * Normalize -> RandomErasing, as torchvision defines the ops on FLOAT tensors in [0, 1] (no rounding to 8 bits between the ops; the
 * reference's PIL pipeline rounds after every op -- the stated deviation, at most one 8-bit step per op).
 *
 * Parameter table: SPV_AUG_NPARAM fp32 per sample,
 *   [SPV_AUG_FLIP] 0 / 1                   [SPV_AUG_BRIGHT] [SPV_AUG_CONTRAST] [SPV_AUG_SAT] blend factors (1 = identity)
 *   [SPV_AUG_HUE] hue shift in turns (0 = skipped)       [SPV_AUG_ORDER] 0..23: the order of the four jitter ops, the index of the
 *   permutation of (brightness, contrast, saturation, hue) in lexicographic order (0 = b c s h, 23 = h s c b)
 *   [SPV_AUG_GRAY] 0 / 1                   [SPV_AUG_ANGLE] rotation in DEGREES (0 = skipped; the kernel takes cos and sin itself)
 *   [SPV_AUG_BLUR] 0 / 1, [SPV_AUG_SIGMA]  [SPV_AUG_ERASE_I / _J / _H / _W] top, left, height, width of the erased rectangle
 *   (height 0 or width 0 = none); entries 14 and 15 are written zero and not read.
 *
 * spv_augment_params fills the table on the device, one thread per sample, from the library's counter hash (the mix32 of the dropout
 * masks) keyed by (seed, step, sample slot, draw index): no host synchronisation, no torch generator.  The stream of numbers is the
 * library's own, not torchvision's.  Draw indices: 0 flip, 1-3 brightness / contrast / saturation, 4 hue, 5 order, 6 grayscale,
 * 7 angle, 8 blur, 9 sigma, 10 erase, then for attempt a < 10 of RandomErasing's search 11 + 4 a: area, log-ratio, top, left
 * (h = round(sqrt(area ratio)), w = round(sqrt(area / ratio)), accepted when h < H and w < W, top-left uniform on the positions that keep it inside; none accepted = no erase).
 * Every Bernoulli is "uniform < p", every range [lo, hi] is lo + (hi - lo) u: p = 0 or lo == hi switches a draw off. */
#define SPV_AUG_NPARAM 16
#define SPV_AUG_FLIP 0
#define SPV_AUG_BRIGHT 1
#define SPV_AUG_CONTRAST 2
#define SPV_AUG_SAT 3
#define SPV_AUG_HUE 4
#define SPV_AUG_ORDER 5
#define SPV_AUG_GRAY 6
#define SPV_AUG_ANGLE 7
#define SPV_AUG_BLUR 8
#define SPV_AUG_SIGMA 9
#define SPV_AUG_ERASE_I 10
#define SPV_AUG_ERASE_J 11
#define SPV_AUG_ERASE_H 12
#define SPV_AUG_ERASE_W 13
typedef struct spv_augment_cfg {   /* a HOST struct, read during the call */
    float flip_p;
    float bright_lo, bright_hi, contrast_lo, contrast_hi, sat_lo, sat_hi, hue_lo, hue_hi;
    float gray_p;
    float degrees;                 /* angle U[-degrees, degrees] */
    float blur_p, sigma_lo, sigma_hi;
    float erase_p, scale_lo, scale_hi, ratio_lo, ratio_hi;
} spv_augment_cfg;
int spv_augment_params(float* params, int batch, int chans, int height, int width, const spv_augment_cfg* cfg, uint64_t seed,
                       uint64_t step, void* stream);
/* 1 when spv_augment_u8 can stage the image: chans 1 or 3, height and width >= 2, and two fp32 copies of the image within the 64 KiB
 * of LDS a workgroup may take (3 x 32 x 32 and 1 x 28 x 28 fit; 224 x 224 does not: spv_augment_tiled_u8 below takes it). */
int spv_augment_supported(int chans, int height, int width);
/* Applies the chain: out_nchw[b] (fp32 [chans][height][width], normalised) from src_nhwc[index[b]] (uint8 [height][width][chans], the
 * loader's layout as spv_patchify_u8 takes it; index == NULL: rows 0..batch-1) and params[b].  A pure function of its arguments.
 * Per image, on floats: u8 / 255 mirrored in W if flip; the four jitter ops in the drawn order, each clamped to [0, 1] (brightness
 * x b; contrast c x + (1 - c) mean(grey); saturation s x + (1 - s) grey; hue by torchvision's hexcone RGB <-> HSV round trip, h :=
 * frac(h + shift)), grey = 0.2989 R + 0.587 G + 0.114 B (chans == 1: grey = the pixel, saturation and hue the identity); grayscale;
 * nearest-neighbour rotation about (W/2, H/2) with zero fill; separable 3-tap Gaussian blur with reflect padding; (x - mean[c])
 * inv_std[c]; erased rectangle := 0.  DESIGN.md section 4c has the formulas.
 * An index outside [0, n_src) cannot be seen by the host (the index lives on the device, and calls never synchronise): the kernel
 * reads nothing for such a row and writes NaN to its whole image. */
int spv_augment_u8(const unsigned char* src_nhwc, const int64_t* index, const float* params, const float* mean, const float* inv_std,
                   float* out_nchw, int batch, int n_src, int chans, int height, int width, void* stream);
/* The same chain on output tiles, for images spv_augment_u8 cannot stage (64 x 64 ... 224 x 224 ... 512 x 512): same definition,
 * parameter table and random stream; every pixel comparable with tests/augment_ref.py under the same rule.
 * spv_augment_plan: 0 = refused by both, 1 = spv_augment_u8 takes it (spv_augment_supported), 2 = only spv_augment_tiled_u8 does.
 * The tiled kernels take chans 1 or 3 and 2 <= height, width <= 512.  The upper bound is one of CORRECTNESS, not of memory: the
 * rotation's nearest-neighbour source coordinate cs X + sn Y + t is evaluated in fp32, whose rounding error grows with the coordinate
 * (about 2^-15 at 512, three terms), and it has to stay far below the 1e-3 window round an integer coordinate inside which the checks
 * treat a pixel as a rounding tie; at 224 the fp32 and float64 floors agree on every pixel outside that window.
 * Two launches per call.  (1) Partial sums of the contrast mean: workgroup (image, chunk of 4096 / width rows) adds the grey values of
 * its pixels after the jitter ops in front of contrast -- fp32 over a thread's <= 16 pixels, a wave, four waves, no atomics -- into
 * workspace[image][chunk]; a sample whose contrast factor is exactly 1 is skipped.  (2) Workgroup (image, 16 x 64 output tile): adds the
 * image's partials in index order in float64 (every tile of an image gets the same bits of the mean), evaluates the chain up to the
 * rotation at each pixel's gathered source position (read from global memory, mirrored if flip), blurs through a one-pixel halo held in
 * LDS when the sample blurs, normalises, erases, stores (16-byte stores when width % 4 == 0 and out_nchw is 16-byte aligned).
 * workspace: spv_augment_tiled_ws_bytes(batch, height, width) bytes (0 for a refused shape), 4-byte aligned, written and read inside
 * the call.  Accepts every shape with plan >= 1 (a 32 x 32 image may be forced through it).  Counts ONE SPV_PATH_AUGMENT per call.
 * Everything else is refused on the host before any launch; an index outside [0, n_src) writes NaN to its image, as above. */
int spv_augment_plan(int chans, int height, int width);
size_t spv_augment_tiled_ws_bytes(int batch, int height, int width);
int spv_augment_tiled_u8(const unsigned char* src_nhwc, const int64_t* index, const float* params, const float* mean,
                         const float* inv_std, float* out_nchw, int batch, int n_src, int chans, int height, int width, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- paired-view distillation: spectre_vit/repl/train.py:92-100, 139-141 (the teacher's view), 300-302, 334-348 (the loss) ------
 * spv_teacher_view_u8: out[b] = Normalize(ToTensor(CenterCrop(crop)(Resize(resize, BICUBIC)(src[index[b]])))) from the resident uint8
 * NHWC set of square n x n images (the layout spv_augment_u8 reads; index == NULL: rows 0..batch-1) to a dense NCHW batch
 * [batch][chans][crop][crop] in `dtype`.  The resize is Pillow's 8-bit resampling (what torchvision's Resize does to a PIL image), bit
 * for bit: per axis, output coordinate xx in [lo, lo + crop), lo = (resize - crop) / 2, has the four taps xmin .. xmin + 3 with integer
 * coefficients k (22 fractional bits, each row summing to 2^22); a pass is clip8((2^21 + sum_d pixel[xmin + d] k[d]) >> 22); the
 * horizontal pass runs first and is stored as uint8, the vertical pass over that.  Only the cropped rows and columns are computed.
 *   table  int32 [5][crop_p], crop_p = crop rounded up to 8: row 0 = xmin, rows 1-4 = the taps, entry j for output coordinate lo + j,
 *          zero past crop (the same table serves both axes); built on the host in float64 (spectre_vit.distillation.teacher_view_table);
 *   lut    fp32 [chans][256]: lut[c][v] = (v / 255 - mean[c]) / std[c] in correctly rounded fp32 operations, i.e. ToTensor + Normalize of
 *          the 8-bit value v (built by the host); bf16 output is that value rounded to nearest even.
 * spv_teacher_view_supported: chans 1 or 3, 2 <= n <= resize (no down-scaling: Pillow widens the support there), 0 < crop <= resize,
 * all four taps of every cropped output inside the image, and the staging of a band of 32 output rows -- table, lut, the source rows
 * the band needs, their horizontal pass -- within the 64 KiB of LDS a workgroup may take (3 x 32 x 32 and 1 x 28 x 28 to 256 / 224 fit,
 * as does 3 x 256 x 256).  Everything else is refused on the host.  An index outside [0, n_src) cannot be seen by the host: the kernel
 * reads nothing for such a row and writes NaN to its whole image.  Table values that become addresses are clamped in the kernel. */
int spv_teacher_view_supported(int chans, int n, int resize, int crop);
int spv_teacher_view_u8(const unsigned char* src_nhwc, const int64_t* index, const int* table, const float* lut, void* out_nchw, int batch,
                        int n_src, int chans, int n, int resize, int crop, int dtype, void* stream);
/* The distillation loss, one launch each way:
 *   out3[0] = w_soft * out3[1] + w_ce * out3[2],   out3[1] = T^2 / rows * sum_r sum_c p_t (log p_t - log p_s),   out3[2] = mean_r CE(z_r, y_r)
 * with p_t = softmax(teacher / T), log p_s = log_softmax(student / T); fp32 logits [rows][classes], int64 labels.  lse3 [3][rows]
 * receives the log-sum-exps of z, z / T and t / T (the backward's input).  log p_t is t / T - lse, so a teacher probability that
 * underflows contributes its limit 0 (log(softmax) gives 0 * -inf = NaN there: the one deviation from the reference's formula).
 * Rows are joined in a fixed order (spv_cross_entropy_fwd's scheme): `workspace` holds spv_distill_loss_workspace_floats() floats,
 * zeroed once by the caller; two calls give the same bits.  A label outside [0, classes) makes out3[0] and out3[2] NaN and reads
 * nothing out of bounds.
 *   dlogits = grad_out[0] / rows * (w_soft T (softmax(z / T) - p_t) + w_ce (softmax(z) - onehot(y))) */
int64_t spv_distill_loss_workspace_floats(void);
int spv_distill_loss_fwd(const float* student, const float* teacher, const int64_t* labels, float* lse3, float* out3, float* workspace,
                         int rows, int classes, float T, float w_soft, float w_ce, void* stream);
int spv_distill_loss_bwd(const float* student, const float* teacher, const int64_t* labels, const float* lse3, const float* grad_out,
                         float* dlogits, int rows, int classes, float T, float w_soft, float w_ce, void* stream);
/* The cached teacher ("cached teacher"): the frozen teacher's logits of every sample, computed once, kept as a
 * dense fp32 matrix cache [n_cache][classes] and read by the sample's index.
 * spv_logit_cache_store: cache[index[r]][:] = logits[r][:] for r < rows (index == NULL: rows 0..rows-1, rows <= n_cache checked on the
 * host).  A row whose index lies outside [0, n_cache) is skipped: nothing is written, nothing is read out of bounds.  16-byte accesses
 * when classes % 4 == 0 and both bases are 16-byte aligned, 4-byte accesses otherwise (10 classes: 40-byte rows).  Plain stores, no
 * atomics: when an index repeats within a call, one of its rows wins.
 * spv_distill_loss_idx_fwd / _bwd: spv_distill_loss_fwd / _bwd with the teacher row of sample r taken at cache + index[r] * classes
 * (index: int64 [rows] on the device).  One device row body, the same grid, workspace and join as the dense entry points: the result is,
 * bit for bit, that of the dense call on the gathered matrix cache[index].  An index outside [0, n_cache) cannot be seen by the host:
 * the kernel reads nothing of the cache for that row; out3[0] and out3[1] become NaN, out3[2] (the cross-entropy) keeps its true value,
 * lse3[2][r] is NaN, and the backward writes NaN to that row of dlogits.  An unfilled cache row (NaN) poisons the loss the same way.
 * Refused on the host, before any launch: a missing pointer, rows / classes / n_cache <= 0, T not positive and finite, a weight not
 * finite.  Counts one SPV_PATH_DISTILL_CACHED per forward launch. */
int spv_logit_cache_store(float* cache, const int64_t* index, const float* logits, int rows, int n_cache, int classes, void* stream);
int spv_distill_loss_idx_fwd(const float* student, const float* cache, const int64_t* index, const int64_t* labels, float* lse3, float* out3,
                             float* workspace, int rows, int n_cache, int classes, float T, float w_soft, float w_ce, void* stream);
int spv_distill_loss_idx_bwd(const float* student, const float* cache, const int64_t* index, const int64_t* labels, const float* lse3,
                             const float* grad_out, float* dlogits, int rows, int n_cache, int classes, float T, float w_soft, float w_ce,
                             void* stream);
/* The feature-matching term of the distillation cell (spectre_vit/repl/train.py:306, 343-346), one launch each way:
 *   out[0] = 1 - mean_r cos_r,   cos_r = s_r . t_r / (|s_r| |t_r|)
 * student [rows][width] in s_dtype, teacher [rows][width] in t_dtype (SPV_F32 or SPV_BF16 each), dense rows.  A wave per row: the three
 * dot products s.s, t.t, s.t are accumulated in fp32 -- lane l takes the 8-element chunks l, l + 64, ... of the row in order, then the
 * lanes 0 .. width % 8 - 1 one element each of what is left -- and joined by the wave reduction; |s| = sqrt(s.s), |t| = sqrt(t.t),
 * cos = (s.t / |s|) / |t|.  The chunks are read as 16-byte loads when both bases and both row pitches are multiples of 16 bytes and as
 * element loads otherwise: the same additions in the same order, the same bits.  stat3 [3][rows] (fp32) receives |s|, |t|, cos: the
 * backward's input.  The one deviation from F.normalize + nn.CosineSimilarity: a row with |s| < 1e-12 or |t| < 1e-12 has cos_r = 0 and
 * a zero gradient row (the reference's clamp_min gives a gradient of order 1e12 there).  A NaN in a row (an unfilled cache row) makes
 * cos_r and out[0] NaN.  Rows are joined in a fixed order (spv_distill_loss_fwd's scheme): `workspace` holds
 * spv_feature_cosine_workspace_floats() floats, zeroed once by the caller; two calls give the same bits.
 *   dstudent_r = -grad_out[0] * w / rows * (t_r / |t_r| - cos_r * s_r / |s_r|) / |s_r|      in s_dtype; elementwise, 4 elements per
 * thread when width % 4 == 0 and the three bases are 16-byte aligned.  `w` is the term's weight in the total loss.
 * spv_feature_cosine_idx_fwd / _idx_bwd: the teacher row of sample r is cache + index[r] * width (cache: fp32 [n_cache][width], index:
 * int64 [rows] on the device).  One device row body, the same grid, workspace and join: the result is, bit for bit, the dense call on
 * cache[index].  An index outside [0, n_cache) cannot be seen by the host: the kernel forms no cache address for that row; its three
 * stat3 entries and out[0] are NaN and the backward writes NaN to that row of dstudent (spv_distill_loss_idx_*'s convention).
 * Refused on the host, before any launch: a missing pointer, rows / width / n_cache <= 0, rows > 2^24, a dtype other than the two, a
 * weight not finite.  No census slot. */
int64_t spv_feature_cosine_workspace_floats(void);
int spv_feature_cosine_fwd(const void* student, const void* teacher, float* stat3, float* out, float* workspace, int rows, int width,
                           int s_dtype, int t_dtype, void* stream);
int spv_feature_cosine_bwd(const void* student, const void* teacher, const float* stat3, const float* grad_out, void* dstudent, int rows,
                           int width, int s_dtype, int t_dtype, float w, void* stream);
int spv_feature_cosine_idx_fwd(const void* student, const float* cache, const int64_t* index, float* stat3, float* out, float* workspace,
                               int rows, int n_cache, int width, int s_dtype, void* stream);
int spv_feature_cosine_idx_bwd(const void* student, const float* cache, const int64_t* index, const float* stat3, const float* grad_out,
                               void* dstudent, int rows, int n_cache, int width, int s_dtype, float w, void* stream);

/* The end of an inference / validation batch, one launch (csrc/spv_infer.hip): logits [rows][classes] (dtype: SPV_F32 or SPV_BF16),
 * labels int64 [rows], *n_valid an int32 DEVICE word (read by the kernel, so a captured launch follows it), 1 <= k <= 8.
 *   pred[r]  int64, every row: the index of the FIRST maximum (torch.argmax's documented tie rule).
 *   stats    spv_eval_head_stats_words() 64-bit words, zeroed by the caller before the first call.  Words 0..2: seen, top1, topk as
 *            int64; word 3: loss_sum as float64; the rest is the kernel's own (partials, arrival counter).  The call ADDS the batch:
 *            only rows with r < *n_valid and 0 <= label < classes count (label -1: predicted, not counted); a row is a top-k hit when
 *            #{j : z_j > z_y} + #{j < y : z_j == z_y} < k (k = 1: pred == y); its loss is logsumexp(z) - z_y in fp32, max-subtracted.
 * The batch is joined in a fixed order and added to loss_sum with one float64 add: the same calls give the same bits. */
int64_t spv_eval_head_stats_words(void);
int spv_eval_head(const void* logits, const int64_t* labels, const int* n_valid, int64_t* pred, void* stats, int rows, int classes, int k,
                  int dtype, void* stream);

/* ---- the training meter: the loss forwards that also keep the training loop's books (spectre_vit/repl/train.py:221-224, 243 and, in
 * the distillation cell, :329-332, 355-361) -- hits counted on the row walk the loss already does, the step's scalars written into a
 * device-resident log, so that a (graph-replayed) step records itself and an epoch costs ONE host read.  DESIGN.md section 4h.
 *
 * The meter is ONE contiguous block of spv_train_meter_words(capacity) 64-bit words, 8-byte aligned, laid out like spv_eval_head's
 * stats block.  The caller zeroes it and writes `capacity` before the first call (and to start a new epoch):
 *   word 0  cursor    steps logged so far = the log row the next step writes
 *   word 1  capacity  log rows the block holds (written by the caller, only read by the kernels)
 *   word 2  dropped   steps that found the log full (cursor == capacity): no row written, totals still accumulated
 *   word 3-5  seen, top1, topk   int64: rows with a label in [0, classes), and the top-1 / top-k hits among them, over all steps
 *   word 6-8  loss_sum, soft_sum, ce_sum   float64 bits: the sums of the steps' fp32 loss (soft term, CE term), one add per step
 *   word 9-15 reserved, zero
 *   then `capacity` log rows of SPV_TRAIN_METER_ROW words, one per step: the step's loss, soft and CE as fp32 bits in the low half of a
 *   word each (soft and CE are 0 on the plain cross-entropy path), then the step's top1 and topk counts.
 * pred, the top-1 hit and the top-k hit are spv_eval_head's, on the (student) logits: first maximum (a NaN entry never wins; a row
 * without an ordered maximum predicts class 0), and #{j : z_j > z_y} + #{j < y : z_j == z_y} < k.  A row whose label is outside
 * [0, classes) is not counted in seen / top1 / topk; it makes the step's loss NaN exactly as in the un-metered call, and that NaN goes
 * into its log row and into loss_sum (what a host's `running += loss` does).
 * loss, lse (out3, lse3) are, bit for bit, those of the un-metered entry point on the same inputs: the same grid, the same partial
 * order, the same join.  The last workgroup to arrive also joins the workgroups' hit counts, writes log row `cursor`, adds to the
 * totals, advances the cursor and re-arms the counter; a full log advances `dropped` instead of writing.  Nothing is written past the
 * block.  The row index is read from the device, so a captured launch logs a new row at every replay.
 * Arguments: those of the un-metered entry point, then meter, k (1..8), then the stream.  workspace: the *_meter_workspace_floats() of
 * the entry point (the un-metered workspace, then the workgroups' hit counts), zeroed once by the caller.
 * Refused on the host, before any launch: a null meter or one not 8-byte aligned, k outside 1..8, rows outside 1..2^24 or classes
 * outside 1..2^24-1 (counts and class indices are joined as exact fp32 integers), and what the un-metered entry point refuses.
 * spv_train_meter_words returns 0 (and sets spv_last_error) for a capacity outside 1..SPV_TRAIN_METER_MAX_CAPACITY. */
#define SPV_TRAIN_METER_HEADER 16
#define SPV_TRAIN_METER_ROW 5
#define SPV_TRAIN_METER_MAX_CAPACITY (1 << 24)
int64_t spv_train_meter_words(int64_t capacity);
int64_t spv_cross_entropy_meter_workspace_floats(void);
int spv_cross_entropy_meter_fwd(const float* logits, const int64_t* labels, float* lse, float* loss, float* workspace, int rows,
                                int classes, void* meter, int k, void* stream);
int64_t spv_distill_loss_meter_workspace_floats(void);
int spv_distill_loss_meter_fwd(const float* student, const float* teacher, const int64_t* labels, float* lse3, float* out3, float* workspace,
                               int rows, int classes, float T, float w_soft, float w_ce, void* meter, int k, void* stream);
int spv_distill_loss_idx_meter_fwd(const float* student, const float* cache, const int64_t* index, const int64_t* labels, float* lse3,
                                   float* out3, float* workspace, int rows, int n_cache, int classes, float T, float w_soft, float w_ce,
                                   void* meter, int k, void* stream);

/* ---- the resident loader: DataLoader(shuffle=True) of spectre_vit/repl/train.py:147-155, 216-218 on the device -- ONE launch reads
 * the step from a device cursor, writes that step's shuffled batch to fixed addresses and advances the cursor, so a captured launch
 * fetches a new batch at every replay and the host feeds a graph-replayed step nothing.  DESIGN.md section 4i.
 *
 * The order (csrc/spv_loader_core.h, host/device; restated in tests/loader_ref.py).  All arithmetic below is on unsigned words.
 *   mix64(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33   (64-bit, murmur3's finaliser)
 *   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16                    (32-bit, the dropout masks')
 *   key(seed, epoch) = mix64(mix64(seed + G) + epoch),  G = 0x9e3779b97f4a7c15
 *   perm_epoch, a bijection of [0, n), 1 <= n < 2^31: a balanced Feistel network on 2 h bits, h the smallest integer >= 1 with
 *   2^(2h) >= n, of SPV_LOADER_ROUNDS = 6 rounds with round keys k_r = the low 32 bits of mix64(key + (r + 1) G), r = 0..5:
 *       (L, R) = (x >> h, x & (2^h - 1));  six times (L, R) := (R, L ^ (mix32(R + k_r) & (2^h - 1)));  x := (L << h) | R
 *   re-applied while x >= n (cycle-walking; 2^(2h) < 4 n, fewer than four passes on average).  shuffle == 0: the identity.
 *   The position rule -- idx[rank::world] cut into batches of `batch`, the tail dropped, the harness's own sharding -- with the step t
 *   taken as the cursor's 64 bits UNSIGNED:  sample r of step t is row  perm_epoch[((t mod S) * batch + r) * world + rank],
 *   epoch = t div S, S = steps_per_epoch with S * batch * world <= n (so S <= (n div world) div batch).  Whatever 64 bits the cursor
 *   holds, every position is < S * batch * world <= n and every row is < n: no source address is formed outside the set.
 *
 * cursor: a block of SPV_LOADER_CURSOR_BYTES (64) bytes, 8-byte aligned, zeroed by the caller: word 0 (64-bit) = the step t, the low
 * half of word 1 = the launch's arrival counter, the rest reserved.  Every workgroup reads t and then adds one to the counter; the
 * last to arrive -- every workgroup holds its copy of t by then -- stores t + 1 and re-arms the counter (the scheme of
 * spv_cross_entropy_fwd's join).  A host that writes the cursor (resume) writes t and zeroes the counter, never under capture.
 *
 * One call writes index[r] = the row (int64 [batch]), labels[r] = labels_src[row] (int64 [batch]; labels_src uint8 or int64 [n], by
 * label_dtype) and the images, from the resident set src_nhwc (uint8 [n][height][width][chans], the layout spv_augment_u8 reads):
 *   SPV_LOADER_FLOAT  img fp32 [batch][chans][height][width] = (x / 255 - mean[c]) * inv_std[c], three fp32 operations, inv_std as the
 *                     caller rounded it (spectre_vit.augment.TrainAugment.norm: 1 / std in float64, rounded once);
 *   SPV_LOADER_UINT8  img uint8 [batch][height][width][chans], the rows copied unchanged (spv_patchify_u8 normalises);
 *   SPV_LOADER_NONE   index and labels only (src_nhwc, img, mean, inv_std unused): the caller hands `index` to spv_augment_u8 or
 *                     spv_distill_loss_idx_fwd.
 * chans 1 or 3, height and width 1..512, any batch: the grid is (image, span of 1024 pixels -- uint8: of 4096 bytes), no whole image
 * in LDS, so 224 x 224 runs like 32 x 32.  Float mode stages a span's bytes in LDS and writes planar rows.  Access width: 16-byte
 * global loads and stores when height * width * chans % 16 == 0, src_nhwc and img are 16-byte aligned and (float mode) height * width
 * % 4 == 0 -- every image, span and plane then starts on a 16-byte boundary; single bytes in and single floats / bytes out otherwise
 * (3 x 5 x 7; a view of the set that starts 4 bytes into its allocation).
 * Refused on the host, before any launch: a null labels_src / cursor / index / labels, a null src_nhwc / img in an image mode, mode
 * float without mean / inv_std, a cursor not 8-byte aligned, n < 1, batch < 1, world < 1 or rank outside [0, world), S < 1 or
 * S * batch * world > n, chans / height / width outside the above, an unknown mode or label dtype, batch * spans >= 2^31. */
#define SPV_LOADER_ROUNDS 6
#define SPV_LOADER_CURSOR_BYTES 64
#define SPV_LOADER_NONE 0
#define SPV_LOADER_FLOAT 1
#define SPV_LOADER_UINT8 2
#define SPV_LOADER_LABEL_U8 0
#define SPV_LOADER_LABEL_I64 1
int64_t spv_loader_cursor_bytes(void);
int spv_loader_fetch(const unsigned char* src_nhwc, const void* labels_src, void* cursor, int64_t* index, int64_t* labels, void* img,
                     const float* mean, const float* inv_std, int n, int batch, int chans, int height, int width, int world, int rank,
                     int steps_per_epoch, uint64_t seed, int shuffle, int mode, int label_dtype, void* stream);
/* Fetch and augment in ONE launch: what spv_loader_fetch(SPV_LOADER_NONE) at the cursor's step t, spv_augment_params(step = t) and
 * spv_augment_u8 do one after the other, bit for bit, with no by-value step -- so a captured launch fetches a new batch AND draws a new
 * table at every replay (the by-value step of spv_augment_params would replay one step's table for ever).  One 256-thread workgroup
 * per image (grid = batch).  Each reads t from the cursor block (the protocol above, groups = batch; the last workgroup to arrive
 * stores t + 1), works the sample's row out with the order above under `loader_seed`, and writes, all at fixed addresses,
 *   index[b], labels[b]   as spv_loader_fetch does;
 *   params[b]             fp32 [batch][SPV_AUG_NPARAM], 16-byte aligned: the sample's table row, drawn with key (augment_seed, t, b)
 *                         exactly as spv_augment_params draws it -- the step's table stays observable;
 *   out_nchw[b]           fp32 [chans][height][width]: spv_augment_u8's chain on src_nhwc[index[b]] with that row.
 * Inside the workgroup the row and the table pass from the threads that work them out to the others through LDS, never through
 * `params`.  Two seeds: under data parallelism the ranks share the loader's seed (one permutation, disjoint parts) and differ in the
 * augmentation's.  cfg is a HOST struct, read during the call.
 * spv_loader_augment_supported: 1 when the kernel can stage the image -- spv_augment_supported's conditions with, on top of its two
 * fp32 copies and reduction slots, 80 bytes of LDS for the step, the row and the table row, and sides <= 512 as the loader asks.  A
 * shape that fills spv_augment_u8's 64 KiB exactly (1 x 89 x 92) is refused; 3 x 32 x 32, 1 x 28 x 28 and 3 x 5 x 7 fit.
 * Refused on the host, before any launch: everything spv_loader_fetch refuses in its float mode (out_nchw as img), everything
 * spv_augment_params refuses (null / misaligned params, null cfg, a probability or range outside its domain, sides < 2), a shape the
 * predicate refuses, out_nchw not 4-byte aligned.  Counts ONE SPV_PATH_AUGMENT per call. */
int spv_loader_augment_supported(int chans, int height, int width);
int spv_loader_fetch_augment(const unsigned char* src_nhwc, const void* labels_src, void* cursor, int64_t* index, int64_t* labels,
                             float* params, float* out_nchw, const float* mean, const float* inv_std, const spv_augment_cfg* cfg, int n,
                             int batch, int chans, int height, int width, int world, int rank, int steps_per_epoch, uint64_t loader_seed,
                             int shuffle, int label_dtype, uint64_t augment_seed, void* stream);
/* The same for the tiled sizes (64 x 64 ... 224 x 224 ... 512 x 512): what spv_loader_fetch(SPV_LOADER_NONE) at the cursor's step t,
 * spv_augment_params(step = t) and spv_augment_tiled_u8 do one after the other, bit for bit in index, labels, params and out_nchw, as
 * TWO launches on `stream`, neither with a by-value step.
 * (1) The pre-pass's grid: 256-thread workgroup (image b, chunk k of 4096 / width rows), batch * parts workgroups.  EVERY workgroup
 *     reads t from the cursor block (the protocol above, groups = batch * parts; the last one to arrive stores t + 1), works out its OWN
 *     sample's row of the set under `loader_seed` and draws its OWN table row with key (augment_seed, t, b) -- both pass to the other
 *     threads through LDS, never through global memory: within a launch a sibling workgroup's writes to `index` / `params` are not
 *     visible -- and writes the partial sum workspace[b][k] with spv_augment_tiled_u8's summation (one definition, the same bits).
 *     Chunk 0 of an image writes index[b], labels[b] and params[b] (16-byte aligned) at their fixed addresses.  A workgroup whose
 *     sample has contrast factor exactly 1 writes no partial but reads t and arrives like every other.
 * (2) spv_augment_tiled_u8's tile kernel, unchanged, on index / params / workspace.
 * spv_loader_augment_tiled_supported: 1 for chans 1 or 3 and 2 <= height, width <= 512 -- the shapes with spv_augment_plan >= 1 inside
 * the loader's sides (a 32 x 32 image may be forced through it; the result is spv_augment_tiled_u8's, not spv_augment_u8's).
 * workspace: spv_augment_tiled_ws_bytes(batch, height, width) bytes, 4-byte aligned, at an address that stays valid while a captured
 * call is replayed.  Refused on the host, before any launch: everything spv_loader_fetch refuses in its float mode (out_nchw as img),
 * everything spv_augment_params refuses, everything spv_augment_tiled_u8 refuses (shape, out_nchw not 4-byte aligned, workspace
 * missing, too small or misaligned, too large a grid).  Counts ONE SPV_PATH_AUGMENT per call. */
int spv_loader_augment_tiled_supported(int chans, int height, int width);
int spv_loader_fetch_augment_tiled(const unsigned char* src_nhwc, const void* labels_src, void* cursor, int64_t* index, int64_t* labels,
                                   float* params, float* out_nchw, const float* mean, const float* inv_std, const spv_augment_cfg* cfg,
                                   int n, int batch, int chans, int height, int width, int world, int rank, int steps_per_epoch,
                                   uint64_t loader_seed, int shuffle, int label_dtype, uint64_t augment_seed, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- state snapshot: a run's device-resident state into one flat staging buffer, by ONE launch ----
 * spv_snapshot_multi copies `bytes` bytes from src to dst for every job, bit for bit, walking a chunk table as spv_adamw_multi does:
 * chunk c is bytes [chunk_off[c], min(chunk_off[c] + chunk_bytes, bytes)) of job chunk_job[c]; one 256-thread workgroup per chunk
 * (grid = nchunks); a job of 0 bytes has no chunk.  jobs / chunk_job / chunk_off / chunk_sum / chunk_nonfinite are device pointers.
 * Any byte count and any source alignment are taken: a chunk whose src and dst are both 16-byte aligned moves 16 bytes per lane and
 * access, one whose two addresses are 4-byte aligned moves 4, any other moves single bytes; a job's last partial 16 bytes (or word) go
 * bytewise.  Nothing outside [dst, dst + bytes) is written.  chunk_off entries and chunk_bytes are multiples of 16 (the host lays the
 * slots out on 256-byte boundaries, so dst never lowers the access width).
 *   chunk_sum[c]        the sum, mod 2^64, of the chunk's bytes read as little-endian 32-bit words counted from the JOB's start, the
 *                       job's last partial word zero-padded.  A job's checksum is the sum of its chunks' sums mod 2^64: integer
 *                       addition makes it independent of chunk_bytes and of any order.  The host folds; no atomics, a fixed layout.
 *   chunk_nonfinite[c]  kind == 1: the whole fp32 words of the chunk whose exponent is all ones (inf, NaN); any other kind: 0.
 * Refused on the host, before any launch: nchunks < 0, chunk_bytes not a positive multiple of 16, and with nchunks > 0 a null table or
 * a null output.  nchunks == 0 launches nothing.  Allocates nothing and synchronises nothing: the call may be captured. */
#define SPV_SNAPSHOT_RAW 0
#define SPV_SNAPSHOT_FP32 1
typedef struct spv_copy_job {
    const void* src;
    void* dst;
    long long bytes;
    int kind;       /* SPV_SNAPSHOT_RAW: raw bytes; SPV_SNAPSHOT_FP32: fp32 values, counted */
    int reserved;
} spv_copy_job;
int spv_snapshot_multi(const spv_copy_job* jobs, const int* chunk_job, const long long* chunk_off, int nchunks, int chunk_bytes,
                       unsigned long long* chunk_sum, int* chunk_nonfinite, void* stream);

/* ---- dataset ingest: a dataset file's pixel payload into the resident set, by ONE launch per uploaded chunk ----
 * src [n][c][h][w] (SPV_DATASET_PLANAR, the CIFAR / MNIST files) or [n][h][w][c] (SPV_DATASET_INTERLEAVED); dst = the other layout,
 * NULL: statistics only.  labels (SPV_LOADER_LABEL_U8 or SPV_LOADER_LABEL_I64 by label_dtype, nullable) feed the histogram.  stats
 * (uint64, spv_dataset_stats_words(c, classes) words, 8-byte aligned, ADDED to: the caller zeroes it once and may call per chunk):
 *   [0, c) sum of x per channel, [c, 2c) sum of x^2, [2c] pixels counted per channel, [2c+1] labels outside [0, classes),
 *   [2c+2, 2c+2+classes) label histogram.  All integer, so the result does not depend on the order of the adds.
 * c in {1, 3}, h, w in 1..512, 0 <= n < 2^31, 0 <= classes <= 2^24; n == 0 launches nothing.  Every byte offset is 64-bit.  src, dst
 * and labels may have ANY alignment: a workgroup stages its unit (a group of whole images of together <= 8192 pixels, or a tile of 8192
 * pixels of a larger image) in LDS at offsets congruent to the global addresses mod 16, moves 16 bytes per lane and access where a
 * run's addresses allow and single bytes at its head and tail, and int64 labels are read bytewise.  Nothing outside
 * [dst, dst + n c h w) is written.  A unit's sums are 32-bit (8192 x 255^2 < 2^32); a workgroup (1024 at the most, each walking
 * every 1024th unit) keeps 64-bit totals over its units and, for classes <= 1024, its label histogram in LDS, and adds them to
 * `stats` once at its end: one 64-bit atomic add per statistic and per class it met (above 1024 classes: one per label).  With c == 1 the two layouts are the same bytes and the call copies.
 * Refused on the host, before any launch: a shape, n, src_layout, label_dtype or classes outside the above, a null or misaligned
 * stats, with n > 0 a null src, and a dst whose bytes overlap src's.  Allocates nothing and synchronises nothing. */
#define SPV_DATASET_PLANAR 0
#define SPV_DATASET_INTERLEAVED 1
int     spv_dataset_ingest(const uint8_t* src, uint8_t* dst, const void* labels, int label_dtype, uint64_t* stats, int64_t n, int c,
                           int h, int w, int src_layout, int classes, void* stream);
int64_t spv_dataset_stats_words(int c, int classes);

#ifdef __cplusplus
}
#endif
#endif /* SPV_H */
