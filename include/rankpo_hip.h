/*
 * rankpo_hip.h -- C ABI of librankpo_hip.so: the MI355X (gfx950) scoring hot path of a
 * contrastive / RankPO embedding trainer.
 *
 * The reference (yflyzhang/RankPO) is pure Python and has no FFI; each entry point below replaces the
 * stock-PyTorch op sequence at the cited reference lines.  Plain device pointers + sizes + a HIP stream;
 * no torch types.  Every call is asynchronous on `stream`, allocates nothing, never synchronises with
 * the host, never throws and never exits: it returns RPO_OK or a negative rpo_status.  All buffers are
 * owned by the caller.  The library keeps no global mutable state and reads no environment variable, so
 * forward may be called from the Python main thread and backward from PyTorch's autograd thread
 * concurrently on different streams, and two callers in one process cannot disagree about a kernel variant.
 *
 * Deviation from SURVEY.md §8b(5), deliberate: there is no `rpo_allgather_qp`.  The cross-device exchange of the
 * path (modeling.py:287-290, 331-404) is ONE rank-major all-gather of a [B + B G, d] block with no arithmetic in it;
 * the RCCL communicator it needs is the one torch.distributed already owns (bootstrap, stream ordering against the
 * caching allocator, async work handles), and a second communicator created behind the C ABI would double RCCL's
 * per-peer xGMI buffers and need its own bootstrap for nothing.  The gather therefore stays on the host side
 * (rankpo_amd/distributed.py: FusedQPGather); what the library contributes to the exchange is that the InfoNCE
 * kernels take the GATHERED matrices plus this rank's row window (q_row0 / q_rows / p_row0 / p_rows below) and
 * write gradients for exactly those rows, which is what removes the backward collective.
 *
 * Embedding matrices are row-major [rows, d] with a contiguous inner dimension; dtype selects the
 * storage type of embeddings / hidden states / scores (f32, bf16 or fp16; accumulation is always f32).
 */
#ifndef RANKPO_HIP_H
#define RANKPO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rpo_stream_t; /* hipStream_t */

typedef enum {
    RPO_OK = 0,
    RPO_ERR_INVALID_ARG = -1,   /* null pointer, non-positive size, bad enum */
    RPO_ERR_UNSUPPORTED = -2,   /* shape / dtype / alignment this build does not handle */
    RPO_ERR_WORKSPACE = -3,     /* workspace too small (see *_workspace_bytes) */
    RPO_ERR_LAUNCH = -4         /* hipGetLastError() != hipSuccess after the launch */
} rpo_status;

typedef enum { RPO_DT_F32 = 0, RPO_DT_BF16 = 1, RPO_DT_F16 = 2 } rpo_dtype;
typedef enum { RPO_POOL_LAST = 0, RPO_POOL_CLS = 1 } rpo_pool_mode;
/* INBATCH: scores [Q,P], target_i = i * (P / Q)  (modeling.py:292-302)
 * FIRST:   scores [Q,G] with G = P / Q, row i scored against p rows i*G .. i*G+G-1, target 0 (305-311) */
typedef enum { RPO_TARGET_INBATCH = 0, RPO_TARGET_FIRST = 1 } rpo_target_mode;
typedef enum { RPO_LOSS_SIGMOID = 0, RPO_LOSS_HINGE = 1 } rpo_loss_type;

int rpo_version(void);
/* What this build of the library contains beyond the default: a bit set of rpo_build_flag.  RPO_BUILD_ONEWAVE64: the head_dim-64
 * one-wave-per-SIMD attention kernels (q_block = 64 at head_dim 64 in rpo_flash_attn_fwd / _bwd; `make ONEWAVE64=1`).  They are
 * correct and measured 4-10 % slower than the default kernels at head_dim 64, so the default build answers RPO_ERR_UNSUPPORTED there. */
typedef enum { RPO_BUILD_ONEWAVE64 = 1 } rpo_build_flag;
int rpo_build_flags(void);
const char* rpo_status_string(int status);
/* hipGetErrorString of the HIP error behind the calling thread's most recent RPO_ERR_LAUNCH (diagnostics). */
const char* rpo_last_hip_error(void);

/* ---------------------------------------------------------------------------------------------
 * (1) pooling + L2 normalisation.
 * Replaces modeling.py:224-236 (== rankpo_trainer.py:409-417, modeling.py:523-534):
 *   idx_n = (argmin_l mask[n,l] - 1) mod L   (first index of the row minimum; RPO_POOL_LAST)
 *        or 0                                  (RPO_POOL_CLS, modeling.py:231-232)
 *   x_n = h[n, idx_n, :];  out_n = normalize ? x_n / max(||x_n||_2, eps) : x_n
 * h: [N, L, d] with element strides (h_stride_n, h_stride_l, 1).  mask: int64 [N, L] contiguous
 * (may be NULL for RPO_POOL_CLS).  Saved for backward: idx_out int32 [N], norm_out f32 [N] (= ||x_n||).
 * --------------------------------------------------------------------------------------------- */
int rpo_pool_normalize_fwd(const void* h, int64_t h_stride_n, int64_t h_stride_l, const int64_t* mask,
                           int64_t N, int64_t L, int64_t d, int dtype, int pool_mode, int normalize,
                           float eps, void* out, int32_t* idx_out, float* norm_out, rpo_stream_t stream);

/* Backward of (1) (autograd of index-select + F.normalize).  grad_out, out: [N, d].
 *   dx_n = normalize ? (norm_n >= eps ? (g_n - out_n <out_n, g_n>) / norm_n : g_n / eps) : g_n
 * If dh != NULL the dense gradient [N, L, d] (contiguous) is written IN FULL: zeros everywhere except
 * row idx_n of sample n (one pass; replaces zeros() + index_put_).  If drow != NULL, dx is also
 * written as [N, d] (for callers that scatter themselves).  At least one of them must be non-NULL. */
int rpo_pool_normalize_bwd(const void* grad_out, const void* out, const int32_t* idx, const float* norm,
                           int64_t N, int64_t L, int64_t d, int dtype, int normalize, float eps,
                           void* dh, void* drow, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (2) similarity + temperature + InfoNCE cross-entropy, fused.
 * Replaces modeling.py:292-314 (training) and :321 (eval: pass lse_out = loss_out = NULL, temperature 1).
 *   INBATCH: scores[i,j] = <q_i, p_j> / T                      [Q, P]
 *   FIRST:   scores[i,g] = <q_i, p_{iG+g}> / T                  [Q, G]
 *   lse_i = log sum_j exp(scores[i,j]);  loss = mean_i (lse_i - scores[i, target_i])
 * scores_out has the storage dtype; with bf16 storage the rounding points are the reference's
 * (dot -> bf16, / T -> bf16) and lse / loss are computed in f32 from the stored (rounded) scores.
 * lse_out f32 [Q], loss_out f32 [1].  workspace: rpo_infonce_workspace_bytes(), 256-byte aligned.
 * --------------------------------------------------------------------------------------------- */
size_t rpo_infonce_workspace_bytes(int64_t Q, int64_t P, int64_t d, int dtype);

int rpo_infonce_fwd(const void* q, const void* p, int64_t Q, int64_t P, int64_t d, int dtype,
                    float temperature, int target_mode, void* scores_out, float* lse_out, float* loss_out,
                    void* workspace, size_t workspace_bytes, rpo_stream_t stream);

/* Fault injection for the tests (not on the hot path): sets every arrival-counter slot of the multi-block single-launch
 * forward (Q <= 64 with several blocks, e.g. the 64 x 384 matrix of 8 ranks) to `word`, as a launch that never finished
 * would leave it.  The next rpo_infonce_fwd must still write lse and loss (the slots are epoch-stamped). */
int rpo_infonce_debug_poison_tickets(uint64_t word, rpo_stream_t stream);

/* Backward of (2): gradients of grad_loss[0] * loss with respect to the caller's OWN rows only
 * (q rows [q_row0, q_row0 + q_rows), p rows [p_row0, p_row0 + p_rows)): with cross-device negatives
 * the other rows of the gathered matrices are constants (modeling.py:374-377), so nothing else is
 * needed and no backward collective exists.  grad_loss: device f32 scalar.  dq_out [q_rows, d],
 * dp_out [p_rows, d] in the storage dtype.  Either output may be NULL (then it is skipped). */
int rpo_infonce_bwd(const void* q, const void* p, const void* scores, const float* lse,
                    const float* grad_loss, int64_t Q, int64_t P, int64_t d, int dtype, float temperature,
                    int target_mode, int64_t q_row0, int64_t q_rows, int64_t p_row0, int64_t p_rows,
                    void* dq_out, void* dp_out, void* workspace, size_t workspace_bytes, rpo_stream_t stream);

/* GEMM form of the backward for large Q*P (in-batch mode): writes the softmax gradient itself,
 *   ds_out  [q_rows, P] = dS[q_row0 .. , :]      and      dst_out [p_rows, Q] = (dS[:, p_row0 ..])^T
 * with dS[i,j] = grad_loss/(Q T) (exp(S[i,j] - lse_i) - [j == i (P/Q)]), in the storage dtype, so that
 * dq = ds_out @ p and dp = dst_out @ q are two plain library GEMMs (hipBLASLt via the caller).  Either output
 * may be NULL. */
int rpo_infonce_ds(const void* scores, const float* lse, const float* grad_loss, int64_t Q, int64_t P, int dtype,
                   float temperature, int64_t q_row0, int64_t q_rows, int64_t p_row0, int64_t p_rows,
                   void* ds_out, void* dst_out, rpo_stream_t stream);

/* The two products of that GEMM form on the FORWARD kernel's own MFMA frame (round 5; replaces autograd's
 * `grad_scores @ p` / `grad_scores.t() @ q` of modeling.py:252's matmul, which rounds 1-4 handed to hipBLASLt):
 *   C [rows_b, rows_a] = B [rows_b, K] A [rows_a, K]^T      bf16 in, f32 accumulation, one rounding to bf16
 * 256 x 256 tiles, K-step 64, 16-byte LDS-DMA staging, phased MFMA schedule (sim_tile256_kernel with a plain epilogue).
 * Both operands are contiguous along the reduction, as q and p are in the forward:
 *   dq [q_rows, d] = rpo_sim_gemm_nt(a = p_all^T [d, P], b = ds_out  [q_rows, P], K = P)
 *   dp [p_rows, d] = rpo_sim_gemm_nt(a = q_all^T [d, Q], b = dst_out [p_rows, Q], K = Q)
 * with the transposed embeddings from rpo_transpose.  lda / ldb / ldc: row strides in elements.  Requires K % 64 == 0,
 * strides % 8 == 0 and 16-byte aligned pointers (RPO_ERR_UNSUPPORTED otherwise: the caller keeps the library GEMM). */
int rpo_sim_gemm_nt(const void* a, int64_t rows_a, int64_t lda, const void* b, int64_t rows_b, int64_t ldb, int64_t K,
                    void* c, int64_t ldc, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (3) RankPO paired scoring + loss + metrics.
 * Replaces rankpo_trainer.py:436-443 (scores), 545-566 (rankpo_loss), 482-520 (loss mix + metrics).
 *   scores[b,g] = <q_b, p_{2b+g}>   (g = 0 chosen, 1 rejected; unscaled)
 *   adv = (c - r) - (reference_free ? 0 : ref_c - ref_r);  logits = adv / T - gamma_beta_ratio
 *   sigmoid: -logsig(beta z)(1 - eps) - logsig(-beta z) eps ;  hinge: relu(1 - beta z)
 *   loss = rankpo_weight * mean(losses) [if > 0] + sft_weight * CE(scores / T, 0) [if > 0]
 * ref_chosen / ref_rejected: f32 [B] or NULL (no reference model -> 0).  Outputs (all f32):
 * scores_out [B,2], losses_out [B], loss_out [1], metrics_out [RPO_NUM_METRICS], dscores_out [B,2]
 * (= d loss / d scores, consumed by rpo_rankpo_bwd).
 * --------------------------------------------------------------------------------------------- */
typedef struct {
    float beta;
    float temperature;
    float gamma_beta_ratio;
    float label_smoothing;
    float rankpo_weight;
    float sft_weight;
    int32_t loss_type;      /* rpo_loss_type */
    int32_t reference_free; /* 0 / 1 */
} rpo_rankpo_params;

enum {
    RPO_METRIC_RANKPO_LOSS = 0,      /* valid iff rankpo_weight > 0 */
    RPO_METRIC_SFT_LOSS = 1,         /* valid iff sft_weight > 0 */
    RPO_METRIC_REWARDS_CHOSEN = 2,   /* mean beta (c - ref_c) */
    RPO_METRIC_REWARDS_REJECTED = 3,
    RPO_METRIC_REWARDS_ACCURACIES = 4,
    RPO_METRIC_REWARDS_MARGINS = 5,
    RPO_METRIC_SCORES_CHOSEN = 6,
    RPO_METRIC_SCORES_REJECTED = 7,
    RPO_METRIC_SCORES_MARGINS = 8,
    RPO_NUM_METRICS = 9
};

int rpo_rankpo_fwd(const void* q, const void* p, const float* ref_chosen, const float* ref_rejected,
                   int64_t B, int64_t d, int dtype, const rpo_rankpo_params* params, float* scores_out,
                   float* losses_out, float* loss_out, float* metrics_out, float* dscores_out,
                   rpo_stream_t stream);

/* dq_b = gl (ds[b,0] p_{2b} + ds[b,1] p_{2b+1});  dp_{2b+g} = gl ds[b,g] q_b;  gl = grad_loss[0]. */
int rpo_rankpo_bwd(const void* q, const void* p, const float* dscores, const float* grad_loss, int64_t B,
                   int64_t d, int dtype, void* dq_out, void* dp_out, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (4) "next" row f2: flat-buffer AdamW step (replaces the DeepSpeed ZeRO-1 bf16 optimizer step the reference
 * scripts configure: configs/ds_zero1_config_llama.json, scripts/train/run_contrastive.sh:33-40).
 * torch.optim.AdamW semantics on n elements (n % 4 == 0, 16-byte aligned buffers):
 *   g = grad * (grad_scale ? grad_scale[0] : 1);  w *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
 *   w -= (lr / bias_corr1) * m / (sqrt(v) / sqrt(bias_corr2) + eps)
 * dtype = storage type of param and grad (RPO_DT_F32 / RPO_DT_BF16; fp16: rpo_adamw_step_scaled below).  bf16 params need an f32 `master` copy (updated, then rounded into
 * param); for f32 params master may be NULL.  grad_scale: device f32 scalar or NULL (clip / 1/GAS factor).
 * rpo_sumsq_partial: partial_out[b] = sum of squares of block b's share of x (for the global grad norm).
 * --------------------------------------------------------------------------------------------- */
int rpo_adamw_step(void* param, float* master, const void* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   int dtype, float lr, float beta1, float beta2, float eps, float weight_decay,
                   float bias_corr1, float bias_corr2, const float* grad_scale, rpo_stream_t stream);
int rpo_sumsq_partial(const void* x, int64_t n, int dtype, float* partial_out, int nblocks, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (4b) fp16 training: dynamic loss scaling on the device + the AdamW step that obeys it.  Stands where the reference's
 * fp16 BGE run has DeepSpeed's DynamicLossScaler (configs/ds_zero1_config_bge.json:2-11: loss_scale 0, initial_scale_power 16,
 * loss_scale_window 1000, hysteresis 2, consecutive_hysteresis false, min_loss_scale 1).  No value visits the host.
 *
 * rpo_sumsq_partial takes RPO_DT_F16 for this (it answered RPO_ERR_INVALID_ARG before; nothing else about it changed).  The sum
 * of its partials is the overflow check: squares of finite fp16 values summed in f32 cannot overflow for any buffer that fits
 * in memory, so the sum is non-finite exactly when some gradient element is inf or NaN.
 *
 * State block: RPO_LS_WORDS 32-bit words in device memory, 16-byte aligned, indexed by rpo_ls_word.  SCALE, MULT and NORM are
 * f32, the others int32.  Initial state: SCALE = 2^initial_scale_power (or the static scale), CUR_HYSTERESIS = hysteresis,
 * everything else 0.  Words 9..15 are reserved (zero).
 *
 * rpo_loss_scale_update (one launch, one working thread): sumsq = device scalar, the sum of squares of the SCALED accumulated
 * gradient (after the rank all-reduce when the optimizer state is partitioned); pre_scale = 1 / GAS / world; max_grad_norm <= 0:
 * no clipping.  With s = SCALE on entry:
 *   SKIP = sumsq is inf or NaN;  NORM = sqrt(sumsq) pre_scale / s;
 *   MULT = pre_scale / s * min(1, max_grad_norm / (NORM + 1e-6))   (0 when SKIP; NORM and MULT are computed in f64, rounded once)
 *   SKIP:  SKIPPED_STEPS += 1; and when dynamic:  FLOOR_HITS += 1 if s <= min_scale (DeepSpeed raises there; here it is counted);
 *          if hysteresis == 1 or CUR_HYSTERESIS == 1: SCALE = max(s / 2, min_scale)   else: CUR_HYSTERESIS -= 1;   GOOD_STEPS = 0
 *   else:  APPLIED_STEPS += 1; and when dynamic:  GOOD_STEPS += 1;  if consecutive_hysteresis: CUR_HYSTERESIS = hysteresis;
 *          if GOOD_STEPS % window == 0: { if !consecutive_hysteresis: CUR_HYSTERESIS = hysteresis;  SCALE = 2 s }
 * dynamic == 0 is a static scale: SCALE, GOOD_STEPS and CUR_HYSTERESIS stay, an overflow still skips the step.
 * window >= 1, hysteresis >= 1, pre_scale > 0, min_scale > 0 (RPO_ERR_INVALID_ARG otherwise).
 *
 * rpo_adamw_step_scaled: rpo_adamw_step for RPO_DT_F16 parameters and gradients with an f32 master (required), m and v --
 * 28 B/element as bf16 -- driven by the state block as rpo_loss_scale_update left it: SKIP != 0 writes NOTHING; otherwise
 * g = grad * MULT, bias_corr1 = 1 - beta1^APPLIED_STEPS and bias_corr2 likewise (f64 powers of the f32 betas as passed, rounded to f32 once), and the
 * stored parameter is the round-to-nearest-even fp16 of the new master.  Other dtypes: RPO_ERR_UNSUPPORTED (rpo_adamw_step
 * serves them).
 * --------------------------------------------------------------------------------------------- */
typedef enum {
    RPO_LS_SCALE = 0,            /* f32  loss scale the NEXT backward runs under */
    RPO_LS_MULT = 1,             /* f32  factor on the stored gradient in this step's AdamW */
    RPO_LS_NORM = 2,             /* f32  unscaled global gradient norm of this step (non-finite when skipped) */
    RPO_LS_SKIP = 3,             /* i32  1: this step's gradient overflowed, AdamW writes nothing */
    RPO_LS_GOOD_STEPS = 4,       /* i32  steps without overflow since the last one */
    RPO_LS_CUR_HYSTERESIS = 5,   /* i32 */
    RPO_LS_APPLIED_STEPS = 6,    /* i32  steps AdamW applied: the bias-correction step count */
    RPO_LS_SKIPPED_STEPS = 7,    /* i32 */
    RPO_LS_FLOOR_HITS = 8,       /* i32  overflows met at SCALE <= min_scale */
    RPO_LS_WORDS = 16
} rpo_ls_word;
int rpo_loss_scale_update(const float* sumsq, void* ls_state, float pre_scale, float max_grad_norm, int dynamic, int window,
                          int hysteresis, int consecutive_hysteresis, float min_scale, rpo_stream_t stream);
int rpo_adamw_step_scaled(void* param, float* master, const void* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          int dtype, float lr, float beta1, float beta2, float eps, float weight_decay, const void* ls_state,
                          rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (5) fused elementwise pieces of the Llama block used by rankpo_amd/encoder.py (the encoder itself stays under
 * PyTorch-ROCm).  16-byte aligned; element counts multiples of 16 / sizeof(elem).
 *   rpo_swiglu_fwd: out = silu(g) * u                   (replaces F.silu + mul of HF LlamaMLP).  g, u: [rows, cols]
 *     with row stride ld_gu elements (g and u may be the two halves of ONE fused gate|up projection output: u = g + cols,
 *     ld_gu = 2 cols); out: [rows, cols] with row stride ld_out.
 *   rpo_swiglu_bwd: dg = dout * u * silu'(g), du = dout * silu(g); dg / du with row stride ld_dgu (again possibly the
 *     two halves of one [rows, 2 cols] buffer).  prod_out (may be NULL): also writes silu(g) * u, row stride ld_prod --
 *     the recomputed forward product that the weight gradient of the following projection needs; prod_out == dout is
 *     allowed (every element of dout is read before it is overwritten), which makes the recompute free of extra traffic.
 *   rpo_rope: x_out = rot(x_in), both [rows, heads, head_dim] (row stride `row_stride` elements; x_in == x_out allowed), HF
 *     rotate_half convention: (x1, x2) -> (x1 cos - x2 sin, x2 cos + x1 sin) with x1 / x2 the low / high half of each
 *     head; cos_tab / sin_tab: f32 [period, head_dim / 2]; row r uses table row r % period.  backward != 0 applies
 *     the inverse rotation (the gradient of the forward rotation).
 * --------------------------------------------------------------------------------------------- */
int rpo_swiglu_fwd(const void* g, const void* u, void* out, int64_t rows, int64_t cols, int64_t ld_gu, int64_t ld_out,
                   int dtype, rpo_stream_t stream);
int rpo_swiglu_bwd(const void* g, const void* u, const void* dout, void* dg, void* du, void* prod_out, int64_t rows,
                   int64_t cols, int64_t ld_gu, int64_t ld_dout, int64_t ld_dgu, int64_t ld_prod, int dtype,
                   rpo_stream_t stream);
/* rpo_swiglu_bwd with the recomputed product written TRANSPOSED: prod_t_out [cols, rows] (row stride ld_t >= rows), the
 * operand layout in which the weight gradient of the following (down) projection, dW = dY^T prod, has BOTH operands contiguous
 * along the token reduction.  dgu_t_out (may be NULL): dg and du ALSO written transposed, [2 cols, rows] with the same row stride
 * (dg^T in rows 0 .. cols - 1, du^T behind it), the same for the weight gradient of the fused gate|up projection; dg / du are
 * written row-major in any case (the input-gradient GEMM reads them).  The transposed outputs may not overlay the inputs. */
int rpo_swiglu_bwd_t(const void* g, const void* u, const void* dout, void* dg, void* du, void* prod_t_out, void* dgu_t_out,
                     int64_t rows, int64_t cols, int64_t ld_gu, int64_t ld_dout, int64_t ld_dgu, int64_t ld_t, int dtype,
                     rpo_stream_t stream);
int rpo_rope(const void* x_in, void* x_out, int64_t row_stride, const float* cos_tab, const float* sin_tab,
             int64_t rows, int64_t heads, int64_t head_dim, int64_t period, int dtype, int backward,
             rpo_stream_t stream);

/* 2-D transpose out[cols, rows] = in[rows, cols]^T, row-major with row strides ld_in / ld_out (elements); HBM-bound.  Used
 * by the encoder's backward to hand hipBLASLt ONE operand of the weight-gradient GEMM dW = dY^T X (reduction over the
 * tokens) contiguous along the reduction, and W^T to the input-gradient GEMM (stands where PyTorch's autograd of
 * nn.Linear issues `grad_output.t() @ input` / `grad_output @ weight`). */
int rpo_transpose(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, int dtype,
                  rpo_stream_t stream);

/* Residual add + RMSNorm, fused (HF LlamaDecoderLayer: `h = residual + delta; y = rmsnorm(h) * w`).
 *   fwd: x_new = x + delta (delta NULL: x_new = x, x_out unused); rstd_r = rsqrt(mean(x_new_r^2) + eps);
 *        y = x_new * rstd * w.  x, delta, x_out, y: [rows, d]; rstd_out: f32 [rows].
 *   bwd: g = dy * w; c_r = mean(g_r * xhat_r); dx = (g - xhat c) * rstd + dres (dres NULL: no residual gradient);
 *        dw_partial: f32 [rpo_add_rmsnorm_waves(rows), d], one partial sum of dy * xhat per wave (every row of it is
 *        written); the caller sums over the first dimension.
 * d % (16 / sizeof(elem)) == 0, d <= 8192 (bf16) / 4096 (f32) forward, half of that backward. */
int rpo_add_rmsnorm_waves(int64_t rows);
int rpo_add_rmsnorm_fwd(const void* x, const void* delta, const void* weight, float eps, void* x_out, void* y_out,
                        float* rstd_out, int64_t rows, int64_t d, int dtype, rpo_stream_t stream);
int rpo_add_rmsnorm_bwd(const void* dy, const void* x_new, const void* weight, const float* rstd, const void* dres,
                        void* dx_out, float* dw_partial, int64_t rows, int64_t d, int dtype, rpo_stream_t stream);

/* Causal variable-length flash attention, forward, head_dim 64 or 128, bf16, grouped-query heads (encoder side; the packed
 * encoder path of rankpo_amd/encoder.py).  q: [T, num_heads, hd] with token stride q_stride elements (heads contiguous),
 * k / v: [T, num_kv_heads, hd] likewise (all three may be views of one fused projection output).  cu_seqlens: int32
 * [N + 1].  tiles = the query-tile work list, one entry per block of 128 queries, in the format tile_cols names:
 *   2: int32 [ntiles][2] = (sequence id, first query row inside the sequence), heaviest first; one launch block per
 *      (entry, head);
 *   3: int32 [ntiles][3] = (sequence id, first query row, head), ntiles % 8 == 0: launch block b takes entry
 *      (b % 8) * ntiles / 8 + b / 8, so the blocks that share an XCD walk one eighth of the list in order; the caller puts
 *      all entries of one (sequence, kv head) next to each other in one eighth (their K / V then stay in that XCD's L2);
 *      entries whose first query row is >= 2^30 are padding.
 * out: [T, num_heads * hd] (token stride out_stride), lse = log sum_j exp(scale * <q_i, k_j>)
 * over the keys j <= i of the same sequence, f32, laid out [num_heads][T] when lse_max_len == 0 or padded
 * [N][num_heads][lse_max_len] (the layout PyTorch's flash-attention backward reads) when lse_max_len > 0.
 * lse may be NULL: a forward-only caller (ModelForInference.encode, modeling.py:473-554; the RankPO ref_model under
 * inference_mode, rankpo_trainer.py:468-477) -- no row statistics are written, nothing else changes.
 * rope_cos / rope_sin (both NULL, or both f32 [rope_period][hd / 2], 16-byte aligned; token t uses row t % rope_period): q
 * arrives UN-rotated and is rotated IN PLACE (q is written!) by the block that owns each (128 queries x head) piece -- the same
 * arithmetic as rpo_rope -- so that the separate rotary pass only has the k heads left; k must arrive rotated (every query
 * block reads it).  The backward entry point reads the rotated q from memory.
 * q_block = the query rows one work-list entry stands for: 128 (0 means 128), or 64 where (num_heads / num_kv_heads) % 4 == 0: an
 * entry is then 64 queries x the FOUR consecutive q heads that begin at the entry's head (format 3: the head column, a multiple
 * of 4; format 2: one launch block per (entry, group of 4 heads)), which share one kv head -- the one-wave-per-SIMD forward
 * (fa_fwd128w_kernel / fa_fwd64w_kernel); out must be 16-byte aligned and out_stride % 8 == 0 there.  Anything else:
 * RPO_ERR_UNSUPPORTED.  The backward's query list stays a 128-row list either way. */
int rpo_flash_attn_fwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                       int64_t v_stride, const int* cu_seqlens, const int* tiles, int64_t ntiles, int64_t tile_cols,
                       int64_t total_tokens,
                       int64_t num_heads, int64_t num_kv_heads, int64_t head_dim, float scale, void* out,
                       int64_t out_stride, float* lse, int64_t lse_max_len, const float* rope_cos, const float* rope_sin,
                       int64_t rope_period, int64_t q_block, rpo_stream_t stream);

/* Backward of rpo_flash_attn_fwd, head_dim 64 or 128 (two launches: dQ, which also computes the row constants, then dK/dV; no
 * atomics, deterministic).  lse: f32 [num_heads][T] as written by the forward with lse_max_len == 0; delta: f32
 * [2][num_heads][T] scratch (written here: -rowsum(dout * out) and -lse / scale, the initial accumulators of the dP and S
 * chains).  q_tiles as in the forward (q_tile_cols = its format); k_tiles: int32 [n_k_tiles][3] =
 * (sequence id, kv head, first key of a key block); key_block = the number of keys one entry stands for and thereby the dK/dV
 * kernel that consumes the table.  head_dim 64: 256 (one wave per SIMD, entries dealt to the 8 XCDs in equal eighths, padded
 * with first key >= 2^30) or 64 (the 8-wave kernel; entries sorted by (sequence, head, key)); head_dim 128: 128 (one wave per
 * SIMD, 32 keys per wave; table dealt and padded like the 256 one).  Any other value is RPO_ERR_UNSUPPORTED: the meaning of
 * the table is an argument, never process-global state.  sweep_down (key_block 256 and 128; ignored at 64, and when the q-head group
 * is not a power of two): the dK/dV blocks sweep the query slices from the last one downwards, the group's q heads innermost (pairs
 * with a work list that keeps a (sequence, kv head)'s key blocks next to each other: they then read each Q / dO slice at about the
 * same time, once from HBM).  dk / dv differ from the ascending sweep by summation order only; either order is deterministic.
 * dq: [T, num_heads, hd], dk / dv: [T, num_kv_heads, hd] (token strides given), every valid row is written.
 * rope_cos / rope_sin (both NULL, or both f32 [rope_period][hd / 2], 16-byte aligned; token t uses row t % rope_period; the
 * tables rpo_rope rotated q and k with): dq and dk then leave as the gradients w.r.t. the PRE-rotary q / k -- the inverse
 * rotation of rpo_rope(backward = 1) applied in the kernels' epilogues in f32 before the one rounding to bf16, instead of a
 * separate pass over d(q|k).  Not offered with key_block 64 (RPO_ERR_UNSUPPORTED).
 * q_block = the query rows one entry of q_tiles stands for: 128 (0 means 128), or 64 with head_dim 64 and
 * (num_heads / num_kv_heads) % 4 == 0 -- the 64-query x 4-head entries of rpo_flash_attn_fwd's q_block = 64, walked by the
 * one-wave-per-SIMD dQ kernel (fa_bwd_dq64w_kernel; dq 16-byte aligned, dq_stride % 8 == 0).  Anything else: RPO_ERR_UNSUPPORTED. */
int rpo_flash_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, int64_t q_stride,
                       int64_t k_stride, int64_t v_stride, int64_t out_stride, int64_t dout_stride,
                       const int* cu_seqlens, const int* q_tiles, int64_t n_q_tiles, int64_t q_tile_cols, const int* k_tiles,
                       int64_t n_k_tiles, int64_t key_block, int64_t sweep_down, int64_t total_tokens, int64_t num_heads,
                       int64_t num_kv_heads, int64_t head_dim, float scale, const float* lse, float* delta, void* dq, void* dk, void* dv,
                       int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, const float* rope_cos, const float* rope_sin,
                       int64_t rope_period, int64_t q_block, rpo_stream_t stream);

/* One-query-per-sequence attention (rankpo_amd/csrc/lastq_attention.hip): the attention of the LAST block of a last-token-pooled
 * encoder.  The reference pools `last_hidden_state[n, last real token]` (modeling.py:224-230, rankpo_trainer.py:409-413), so the
 * last block's attention output is read for ONE query per sequence -- its last token, which sees every key of its sequence (no
 * mask).  Stands where the packed encoder path called PyTorch's flash-attention op (an AOTriton kernel) with one-row queries.
 *   q: [num_seqs, num_heads, hd] bf16 (sequence stride q_stride elements, heads contiguous) -- already rotated;
 *   k / v: [T, num_kv_heads, hd] packed tokens (token strides k_stride / v_stride; k rotated), cu_seqlens: int32 [num_seqs + 1];
 *   out: [num_seqs, num_heads * hd] bf16; lse: f32 [num_seqs][num_heads] = log sum_j exp(scale <q, k_j>).
 * HBM-bound: K / V are read exactly once (one block per (sequence, kv head) serves the whole query-head group); f32 online
 * softmax, deterministic (fixed merge order, no atomics).  head_dim 64 or 128, num_heads / num_kv_heads in {1, 2, 4}; anything
 * else is RPO_ERR_UNSUPPORTED.
 * Backward: one pass over K / V; writes EVERY row of dk / dv ([T, num_kv_heads, hd], token strides given: e.g. the two halves of
 * one fused d(k|v) buffer) and dq [num_seqs, num_heads, hd]; out / dout / lse as produced / received by the forward. */
int rpo_lastq_attn_fwd(const void* q, int64_t q_stride, const void* k, const void* v, int64_t k_stride, int64_t v_stride,
                       const int* cu_seqlens, int64_t num_seqs, int64_t num_heads, int64_t num_kv_heads, int64_t head_dim,
                       float scale, void* out, int64_t out_stride, float* lse, rpo_stream_t stream);
int rpo_lastq_attn_bwd(const void* q, int64_t q_stride, const void* k, const void* v, int64_t k_stride, int64_t v_stride,
                       const int* cu_seqlens, int64_t num_seqs, int64_t num_heads, int64_t num_kv_heads, int64_t head_dim,
                       float scale, const void* out, int64_t out_stride, const void* dout, int64_t dout_stride, const float* lse,
                       void* dq, int64_t dq_stride, void* dk, void* dv, int64_t dk_stride, int64_t dv_stride, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (9) packed forward of the BERT / XLM-R block (rankpo_amd/csrc/bert_ops.hip; BertEncoder.pooled_cls, used by
 * ModelForInference.encode for CLS-pooled models: modeling.py:231-232, 473-554).  bf16 or fp16 storage (RPO_DT_F32 is
 * RPO_ERR_UNSUPPORTED), f32 arithmetic, one rounding per stored value unless stated otherwise.
 *
 * rpo_bidir_attn_fwd: non-causal variable-length attention over packed tokens (replaces HF BertSelfAttention's
 * softmax(Q K^T scale + mask) V, which the padded path runs as F.scaled_dot_product_attention with a boolean key mask:
 * rankpo_amd/encoder.py BertAttention.forward).  q: [total_q, num_heads, head_dim], k / v: [T_k, num_heads, head_dim], token
 * strides q_stride / k_stride / v_stride elements, heads contiguous (all three may be column blocks of ONE fused q|k|v
 * projection output); out: [total_q, num_heads * head_dim] with token stride out_stride.  cu_seqlens_q / cu_seqlens_k: int32
 * [N + 1], query rows and key rows of sequence n (one table for both is self-attention; cu_seqlens_q = 0, 1, .., N with
 * cu_seqlens_k = the token table is one query per sequence, its CLS row).  tiles: the work list, int32 [ntiles][tile_cols]
 * = (sequence id, first query row inside the sequence) with tile_cols == 2 and q_block == 32 query rows per entry (any other
 * format: RPO_ERR_UNSUPPORTED); one wave per (entry, head).  Scores and the online softmax in f32, P rounded to the storage
 * type for the PV product (as flash attention does), `scale` multiplies the scores.  lse (may be NULL): f32 [num_heads][total_q],
 * natural log.  head_dim 32 or 64, num_heads == num_kv_heads; q / k / v 16-byte aligned with strides % 8 == 0, out 8-byte
 * aligned with out_stride % 4 == 0.  Every sequence length >= 1 works.
 *
 * rpo_add_layernorm_fwd: y = LayerNorm(a + b) * gamma + beta (HF BertSelfOutput / BertOutput: `LayerNorm(dense(h) + input)`;
 * b = the dense output with its bias already added by the GEMM epilogue, a = the residual).  a + b is rounded to the storage
 * type first (the reference's own sum), mean / variance in f32 from it, y rounded once.  b may be NULL (LayerNorm of a).
 * a, b, y: [rows, d] with row strides lda / ldb / ldy (the last block writes N CLS rows through them); gamma / beta [d].
 * d % 8 == 0, d <= 4096, 16-byte aligned, strides % 8 == 0.
 *
 * rpo_gelu_fwd: x = x * 0.5 * (1 + erf(x / sqrt 2)) in place (HF BertIntermediate, hidden_act "gelu"), f32 inside, one
 * rounding; x: [rows, cols], row stride ld; cols % 8 == 0, ld % 8 == 0, 16-byte aligned.
 *
 * rpo_bert_embed_ln_fwd: HF BertEmbeddings.forward on packed tokens: x = (word[ids] + type[token_types]) + pos_emb[pos], rounded
 * to the storage type after each add as the reference's `inputs_embeds + token_type_embeddings; += position_embeddings`, then
 * LayerNorm as above into y [tokens, d] (row stride ldy).  ids / pos / token_types: int32 [tokens]; token_types may be NULL
 * (type 0 for every token).  Tables contiguous [vocab | n_types | n_pos, d]; an index outside its table is clamped into it
 * (the caller checks the ranges).  Same d / alignment rules as rpo_add_layernorm_fwd.
 * --------------------------------------------------------------------------------------------- */
int rpo_bidir_attn_fwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                       const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles, int64_t tile_cols,
                       int64_t q_block, int64_t total_q, int64_t num_heads, int64_t num_kv_heads, int64_t head_dim, int dtype,
                       float scale, void* out, int64_t out_stride, float* lse, rpo_stream_t stream);
int rpo_add_layernorm_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma, const void* beta, float eps,
                          void* y, int64_t ldy, int64_t rows, int64_t d, int dtype, rpo_stream_t stream);
int rpo_gelu_fwd(void* x, int64_t rows, int64_t cols, int64_t ld, int dtype, rpo_stream_t stream);
int rpo_bert_embed_ln_fwd(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word,
                          int64_t vocab, const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos,
                          const void* gamma, const void* beta, float eps, void* y, int64_t ldy, int64_t d, int dtype,
                          rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (9b) f32 storage: the forward of section (9) for an encoder kept in float32 (opt-in: encoder.BERT_NATIVE_F32 /
 * BertEncoder.native_f32, ModelForInference(packed_f32=True)).  Entry points of their own: the entries of (9) keep answering
 * RPO_DT_F32 with RPO_ERR_UNSUPPORTED.  Argument lists of the 16-bit siblings without `dtype`; strides in elements (floats);
 * shapes, work lists, CLS-only mode, status codes as in (9).  No allocation, no host sync, no atomics.  Forward only: the
 * training entries of (10) have no f32 form.
 *
 * rpo_bidir_attn_fwd_f32: the attention of rpo_bidir_attn_fwd on v_mfma_f32_16x16x4_f32: f32 operands, exact f32 products,
 * f32 accumulation; P stays f32 and is never rounded to 16 bits.  The exponent is taken of ((s - m) |scale|) log2(e) with m the
 * running maximum of the raw scores, so no rounding happens at the magnitude of a large score.  lse (may be NULL): f32
 * [num_heads][total_q], natural log.  head_dim 32 or 64, num_heads == num_kv_heads, tile_cols == 2, q_block == 32 (anything
 * else: RPO_ERR_UNSUPPORTED); q / k / v / out 16-byte aligned with strides % 4 == 0.  Every sequence length >= 1 works.
 *
 * rpo_add_layernorm_fwd_f32 / rpo_gelu_fwd_f32 / rpo_bert_embed_ln_fwd_f32: the row kernels of (9) instantiated for float (4
 * elements per 16-byte vector).  a + b and (word + type) + pos are plain f32 adds (nothing to round); two-pass mean / centred
 * variance.  d (cols) % 8 == 0, d <= 4096, 16-byte aligned, strides % 4 == 0.
 * --------------------------------------------------------------------------------------------- */
int rpo_bidir_attn_fwd_f32(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                           const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles,
                           int64_t tile_cols, int64_t q_block, int64_t total_q, int64_t num_heads, int64_t num_kv_heads,
                           int64_t head_dim, float scale, void* out, int64_t out_stride, float* lse, rpo_stream_t stream);
int rpo_add_layernorm_fwd_f32(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma, const void* beta,
                              float eps, void* y, int64_t ldy, int64_t rows, int64_t d, rpo_stream_t stream);
int rpo_gelu_fwd_f32(void* x, int64_t rows, int64_t cols, int64_t ld, rpo_stream_t stream);
int rpo_bert_embed_ln_fwd_f32(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word,
                              int64_t vocab, const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos,
                              const void* gamma, const void* beta, float eps, void* y, int64_t ldy, int64_t d,
                              rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (9c) causal f32 attention of the packed Llama pass (rankpo_amd/csrc/causal_attn_f32.hip; opt-in: encoder.LLAMA_F32_ATTENTION /
 * LlamaEncoder.f32_attention, ModelForInference(f32_attention=True)).  Forward only, for no-grad callers; no allocation, no host
 * sync, no atomics: deterministic.
 *
 * rpo_causal_attn_fwd_f32: causal, grouped-query, variable-length attention over packed tokens on v_mfma_f32_16x16x4_f32, with
 * the numerics of rpo_bidir_attn_fwd_f32 (exact f32 products, f32 accumulation, P never rounded to 16 bits, the exponent taken of
 * ((s - m) |scale|) log2(e) with m the running maximum of the raw scores).  q: [total_q, num_heads, head_dim], k / v: [T_k,
 * num_kv_heads, head_dim], token strides in floats, heads contiguous (column blocks of the fused q|k|v or k|v projection output);
 * out: [total_q, num_heads * head_dim] with token stride out_stride.  Query head h reads kv head h / (num_heads / num_kv_heads).
 * cu_seqlens_q / cu_seqlens_k: int32 [num_seqs + 1]; query i of a sequence with lq queries and lk keys sees key j iff
 * j <= i + (lk - lq) (bottom-right aligned: lq == lk is causal self-attention, lq == 1 is one query over every key).  lq <= lk
 * is the caller's precondition; rows of a sequence that breaks it come out as zeros with lse = -inf where they see no key.
 * tiles: int32 [ntiles][2] = (sequence id, first query row inside the sequence), 32 query rows per entry, the format of
 * rpo_bidir_attn_fwd_f32; one block per (entry, kv head), one wave per query head of the group, K / V steps shared through LDS;
 * key steps past an entry's last visible key are not executed.  lse (may be NULL): f32 [num_heads][total_q], natural log,
 * total_q = cu_seqlens_q[num_seqs] as the kernel reads it.  head_dim 64 or 128; num_heads / num_kv_heads in {1, 2, 4, 8};
 * tile_cols == 2, q_block == 32 (anything else: RPO_ERR_UNSUPPORTED); q / k / v / out 16-byte aligned with strides % 4 == 0.
 * ntiles == 0 is RPO_OK and launches nothing.
 * --------------------------------------------------------------------------------------------- */
int rpo_causal_attn_fwd_f32(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                            const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles,
                            int64_t tile_cols, int64_t q_block, int64_t num_seqs, int64_t num_heads, int64_t num_kv_heads,
                            int64_t head_dim, float scale, void* out, int64_t out_stride, float* lse, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (9d) backward of the causal f32 attention of (9c), for the packed f32 Llama TRAINING pass
 * (rankpo_amd/csrc/causal_attn_f32_bwd.hip; opt-in: encoder.LLAMA_F32_ATTENTION_TRAIN / LlamaEncoder.f32_attention_train,
 * ModelForTraining(f32_attention=True)).  No allocation, no host sync, no atomics: deterministic.
 *
 * rpo_causal_attn_bwd_f32: ONE entry that launches the dQ kernel, then the dK/dV kernel, on the caller's stream, both on
 * v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation, P and dS never rounded to 16 bits).  q / k / v / cu_seqlens_q /
 * cu_seqlens_k / tiles / scale and the visibility rule j <= i + (lk - lq) as in (9c); out: [total_q, num_heads * head_dim], the
 * forward's result, dout: its gradient, lse: f32 [num_heads][total_q], the forward's (required); all token strides in floats,
 * heads contiguous.  k_tiles: int32 [nktiles][2] = (sequence id, first key row inside the sequence), 32 keys per entry (the
 * format of tiles; tile_cols and q_block describe both lists), one entry per 32-key block of every sequence with keys.
 * dq: [total_q, num_heads, head_dim], dk / dv: [T_k, num_kv_heads, head_dim], each with its own token stride (the three may be
 * column blocks of one [T, (num_heads + 2 num_kv_heads) head_dim] buffer).  ws: f32 workspace of 2 * num_heads * total_q
 * floats, required, 16-byte aligned: the dQ kernel leaves (delta = dout . out, 1 / L') per head and query there for the dK/dV
 * kernel, L' the sum of exp(s scale - lse) over the query's visible keys, by which both kernels normalise the probabilities (the
 * rounding of a single-f32 lse cancels; the exponent is taken as in (9c), log2(e) as hi + lo).
 * Summation order: dq[i] sums the keys in ascending order (32-key steps, inside a step by the MFMA's k order); dk[j] / dv[j] sum
 * the query steps of 32 in ascending order from the first query that sees the first key of j's 32-key entry and, inside a
 * step, the query heads of the group in ascending order: ONE chain per element, fixed by the indices alone, so the result is
 * deterministic and depends neither on block scheduling nor on what else is packed in the batch.
 * Zero fill: every dq row of a listed entry and every dk / dv row of a listed key entry is written; keys no query sees (lq == 0)
 * get exact zeros; a query whose lse is -inf contributes exact zeros, never NaN.  No access leaves a sequence.
 * head_dim 64 or 128; num_heads / num_kv_heads in {1, 2, 4, 8}; tile_cols == 2, q_block == 32 (anything else:
 * RPO_ERR_UNSUPPORTED before any launch); q / k / v / out / dout / dq / dk / dv / ws 16-byte aligned with strides % 4 == 0.
 * ntiles == 0 and nktiles == 0 is RPO_OK and launches nothing; an empty list alone skips its kernel.
 * --------------------------------------------------------------------------------------------- */
int rpo_causal_attn_bwd_f32(const void* q, const void* k, const void* v, const void* out, const void* dout, int64_t q_stride,
                            int64_t k_stride, int64_t v_stride, int64_t out_stride, int64_t dout_stride, const float* lse,
                            const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles, const int* k_tiles,
                            int64_t nktiles, int64_t tile_cols, int64_t q_block, int64_t num_seqs, int64_t num_heads,
                            int64_t num_kv_heads, int64_t head_dim, float scale, void* dq, int64_t dq_stride, void* dk,
                            int64_t dk_stride, void* dv, int64_t dv_stride, float* ws, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (9e) causal fp16 attention of the packed Llama pass (rankpo_amd/csrc/causal_attn_f16.hip; opt-in: encoder.LLAMA_FP16_NATIVE /
 * LlamaEncoder.native_fp16, ModelForInference(native_fp16=True): the reference's ModelForInference(use_fp16=True),
 * modeling.py:453-454, for a Llama encoder, whose attention HF runs as softmax(Q K^T / sqrt(d) + causal mask) V).  Forward only,
 * for no-grad callers; no allocation, no host sync, no atomics: deterministic, and a sequence's rows do not depend on what else
 * is packed.
 *
 * rpo_causal_attn_fwd_f16: the contract of (9c) on fp16 storage, in the argument order of rpo_causal_attn_fwd_f32.  q: [total_q,
 * num_heads, head_dim], k / v: [T_k, num_kv_heads, head_dim], fp16, token strides in ELEMENTS, heads contiguous (column blocks of
 * the fused q|k|v or k|v projection output, read as they lie); out: fp16 [total_q, num_heads * head_dim] with token stride
 * out_stride.  Query head h reads kv head h / (num_heads / num_kv_heads).  cu_seqlens_q / cu_seqlens_k: int32 [num_seqs + 1] on
 * the device; query i of a sequence with lq queries and lk keys sees key j iff j <= i + (lk - lq) (bottom-right aligned: lq == lk
 * is causal self-attention, lq == 1 is one query over every key).  lq <= lk is the caller's precondition; rows of a sequence that
 * breaks it come out as zeros with lse = -inf where they see no key.  Masked keys of a step get p = 0 and never enter the
 * running maximum; key steps past an entry's last visible key are not executed; no access leaves the sequence.
 * tiles: int32 [ntiles][2] = (sequence id, first query row inside the sequence), 32 query rows per entry, the format of (9c),
 * built on the host from the lengths; one block per (entry, kv head), one wave per query head of the group, K / V steps staged
 * once per kv head in LDS (V transposed, so that P enters the PV product as it lies in the accumulators).
 * Arithmetic: S and PV on v_mfma_f32_16x16x32_f16 with f32 accumulation; raw scores stay f32 and are never stored as fp16; the
 * scale is applied in f32 (Q is not pre-scaled): p = exp2(((s - m) |scale|) log2(e)) with m the running maximum of the raw
 * scores; P is rounded to fp16 exactly once, as the PV operand, and the row sum adds the same rounded P; the output is divided in
 * f32 and rounded to fp16 once (overflow gives inf).  lse (may be NULL: not written): f32 [num_heads][total_q], natural log,
 * total_q = cu_seqlens_q[num_seqs] as the kernel reads it.
 * head_dim 64 or 128; num_heads / num_kv_heads in {1, 2, 4, 8}; tile_cols == 2, q_block == 32; q / k / v / out 16-byte aligned
 * with token strides % 8 == 0: anything else is RPO_ERR_UNSUPPORTED before any launch.  ntiles == 0 is RPO_OK and launches
 * nothing.
 * --------------------------------------------------------------------------------------------- */
int rpo_causal_attn_fwd_f16(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                            const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles,
                            int64_t tile_cols, int64_t q_block, int64_t num_seqs, int64_t num_heads, int64_t num_kv_heads,
                            int64_t head_dim, float scale, void* out, int64_t out_stride, float* lse, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (9f) backward of the causal fp16 attention of (9e), for the packed fp16 Llama TRAINING pass
 * (rankpo_amd/csrc/causal_attn_f16_bwd.hip; opt-in: encoder.LLAMA_FP16_NATIVE_TRAIN / LlamaEncoder.native_fp16_train,
 * ModelForTraining(native_fp16=True)).  No allocation, no host sync, no atomics: deterministic.
 *
 * rpo_causal_attn_bwd_f16: the contract of (9d) on fp16 storage, in the argument order of rpo_causal_attn_bwd_f32 (no dtype
 * argument).  ONE entry that launches the dQ kernel, then the dK/dV kernel, on the caller's stream.  q / k / v / out / dout /
 * dq / dk / dv are fp16, token strides in fp16 ELEMENTS, heads contiguous; lse: f32 [num_heads][total_q], as
 * rpo_causal_attn_fwd_f16 writes it (required); the visibility rule is j <= i + (lk - lq).  tiles / k_tiles: int32 [n][2], 32 rows
 * per entry, the query and key lists of (9c) / (9d); tile_cols and q_block describe both.  q | k | v and dq | dk | dv may each be
 * column blocks of one fused buffer.  ws: f32 workspace, required: the dQ kernel writes delta = dout . out per head and query
 * there and the dK/dV kernel reads it, so num_heads * total_q floats suffice (half of what (9d) asks for; the signature is
 * (9d)'s).
 * Arithmetic: S, dP and the three gradient products run on v_mfma_f32_16x16x32_f16 with f32 accumulation; raw scores stay f32
 * (never fp16): each 32-wide chunk of the head dim is one MFMA summed from zero and the chunks' f32 sums are added without a
 * rounding, the score carried as an f32 pair into the exponent;
 * p = exp2((s * scale - lse) * log2(e)) with log2(e) carried as hi + lo, as in (9e); no renormalisation by the sum of p (one f32
 * lse at |lse| ~ 60 carries ~4e-6 relative into p, two orders below fp16's 2^-11).  P is rounded to fp16 exactly once, as the
 * operand of dV; dS = p (dP - delta) is formed in f32 and rounded to fp16 exactly once, as the operand of dQ and dK; scale is
 * applied in f32; dq / dk / dv are rounded to fp16 once (overflow gives inf, never a saturated value).  A non-finite dout
 * element reaches the dq row of its query.
 * Summation order: dq[i] sums the keys ascending in 32-key steps; dk[j] / dv[j] sum (query step of 32, query head of the group)
 * ascending from the first query that sees the first key of j's 32-key entry, each (step, head) summed from zero and then added
 * to the running total: the indices alone fix the order, so results are bit-reproducible and do not depend on what else is packed.
 * Zero fill: every dq row of a listed entry and every dk / dv row of a listed key entry is written; keys no query sees (lq == 0)
 * get exact zeros; a query whose lse is -inf contributes exact zeros, never NaN.  No access leaves a sequence (row loads are
 * clamped as in the forward).
 * head_dim 64 or 128; num_heads / num_kv_heads in {1, 2, 4, 8}; tile_cols == 2, q_block == 32; q / k / v / out / dout / dq / dk /
 * dv 16-byte aligned with token strides % 8 == 0: anything else is RPO_ERR_UNSUPPORTED before any launch.  ntiles == 0 and
 * nktiles == 0 is RPO_OK and launches nothing; an empty list alone skips its kernel.
 * --------------------------------------------------------------------------------------------- */
int rpo_causal_attn_bwd_f16(const void* q, const void* k, const void* v, const void* out, const void* dout, int64_t q_stride,
                            int64_t k_stride, int64_t v_stride, int64_t out_stride, int64_t dout_stride, const float* lse,
                            const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles, const int* k_tiles,
                            int64_t nktiles, int64_t tile_cols, int64_t q_block, int64_t num_seqs, int64_t num_heads,
                            int64_t num_kv_heads, int64_t head_dim, float scale, void* dq, int64_t dq_stride, void* dk,
                            int64_t dk_stride, void* dv, int64_t dv_stride, float* ws, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (10) packed TRAINING step of the BERT / XLM-R block (rankpo_amd/csrc/bert_ops.hip; BertEncoder.pooled_cls_train, used by
 * ModelForTraining.embed for CLS-pooled models).  bf16 or fp16 storage (RPO_DT_F32 is RPO_ERR_UNSUPPORTED), f32 arithmetic,
 * no allocation, no host sync, no atomics: deterministic.  Shapes, strides, work lists and alignment as in section (9) unless
 * stated otherwise.
 *
 * Attention-probability dropout: keep(seed, head, packed query row, packed key row) is one stateless counter-based function
 * (Philox2x32-10; counter = (query row, key row >> 2), key = a 32-bit mix of seed and head; each key of a group of 4 reads its own
 * 16-bit field and is kept when field >= round(p_drop * 65536)).  "Packed row" = the row index in q resp. k as passed to the call.
 * 0 <= p_drop < 1; p_drop < 2^-17 takes the kernels without dropout.  The caller folds the layer index into `seed`.
 *
 * rpo_bidir_attn_train_fwd: rpo_bidir_attn_fwd with dropout.  The row sum and lse (required) come from the undropped
 * probabilities P; out = (P o keep / (1 - p_drop)) V.
 *
 * rpo_bidir_attn_bwd: backward of either forward from q, k, v, out, dout, lse -> dq, dk, dv (each strided like its input: all
 * may be column blocks of one fused buffer; 8-byte aligned, strides % 4 == 0; out / dout 16-byte aligned, strides % 8 == 0).
 * Two launches: a dQ kernel, one wave per (q_tiles entry = 32 queries, head), looping over the sequence's keys, and a dK/dV
 * kernel, one wave per (k_tiles entry = (sequence id, first key row inside the sequence), 32 keys, head), looping over the
 * sequence's queries.  delta = rowsum(dout o out) in f32 inside both; P and dS are rounded to the storage type before their MFMA.
 * dP <- keep o dP / (1 - p_drop), dS = P o (dP - delta), dV uses the dropped P.  Every row of dq / dk / dv that a work list covers
 * is written; block_rows == 32, tile_cols == 2.
 *
 * rpo_bidir_attn_dropout_mask: mask[h][i][j] (uint8, 1 = kept) for heads head0 + h < head0 + num_heads, query rows q_row0 + i,
 * key rows k_row0 + j of one sequence's block, from the same device function.  Tests and diagnostics only.
 *
 * rpo_add_layernorm_train_fwd / rpo_bert_embed_ln_train_fwd: the forward entries of section (9), bit for bit, which also store the
 * rounded sum s [rows, d] (row stride lds) that the statistics are taken from.
 *
 * rpo_layernorm_bwd: from s, gamma and dy: mean / rstd recomputed per row in f32 as the forward takes them; ds = rstd (g - mean(g)
 * - xhat mean(g xhat)), g = dy gamma, xhat = (s - mean) rstd: the gradient of BOTH addends.  dgamma_partial / dbeta_partial: f32
 * [rpo_layernorm_bwd_blocks(rows), d], per-block sums of dy xhat / dy in a fixed order (four waves
 * per block, one row per wave at a time, the waves' sums added in wave order); the caller adds the blocks.
 *
 * rpo_gelu_out_fwd: h = gelu(u) out of place (the arithmetic of rpo_gelu_fwd).  rpo_gelu_bwd: du = dh (Phi(u) + u phi(u)), exact
 * erf form, one rounding.
 * --------------------------------------------------------------------------------------------- */
int rpo_bidir_attn_train_fwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                             const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles,
                             int64_t tile_cols, int64_t q_block, int64_t total_q, int64_t num_heads, int64_t num_kv_heads,
                             int64_t head_dim, int dtype, float scale, float p_drop, uint64_t seed, void* out,
                             int64_t out_stride, float* lse, rpo_stream_t stream);
int rpo_bidir_attn_bwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                       const void* out, int64_t out_stride, const void* dout, int64_t dout_stride, const float* lse,
                       const int* cu_seqlens_q, const int* cu_seqlens_k, const int* q_tiles, int64_t n_q_tiles,
                       const int* k_tiles, int64_t n_k_tiles, int64_t tile_cols, int64_t block_rows, int64_t total_q,
                       int64_t num_heads, int64_t num_kv_heads, int64_t head_dim, int dtype, float scale, float p_drop,
                       uint64_t seed, void* dq, int64_t dq_stride, void* dk, int64_t dk_stride, void* dv, int64_t dv_stride,
                       rpo_stream_t stream);
int rpo_bidir_attn_dropout_mask(int64_t q_row0, int64_t k_row0, int64_t len_q, int64_t len_k, int64_t head0, int64_t num_heads,
                                float p_drop, uint64_t seed, unsigned char* mask, rpo_stream_t stream);
int rpo_add_layernorm_train_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma, const void* beta,
                                float eps, void* y, int64_t ldy, void* s, int64_t lds, int64_t rows, int64_t d, int dtype,
                                rpo_stream_t stream);
int rpo_bert_embed_ln_train_fwd(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word,
                                int64_t vocab, const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos,
                                const void* gamma, const void* beta, float eps, void* y, int64_t ldy, void* s, int64_t lds,
                                int64_t d, int dtype, rpo_stream_t stream);
int rpo_layernorm_bwd_blocks(int64_t rows);
int rpo_layernorm_bwd(const void* s, int64_t lds, const void* gamma, const void* dy, int64_t lddy, float eps, void* ds,
                      int64_t ldds, float* dgamma_partial, float* dbeta_partial, int64_t rows, int64_t d, int dtype,
                      rpo_stream_t stream);
int rpo_gelu_out_fwd(const void* u, int64_t ldu, void* h, int64_t ldh, int64_t rows, int64_t cols, int dtype,
                     rpo_stream_t stream);
int rpo_gelu_bwd(const void* u, int64_t ldu, const void* dh, int64_t lddh, void* du, int64_t lddu, int64_t rows, int64_t cols,
                 int dtype, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (10b) hidden-state dropout inside the row kernels of (10) (opt-in: encoder.BERT_FUSED_HIDDEN_DROPOUT, and what gradient
 * checkpointing on the packed step recomputes).  keep(seed, site, row, column) is the attention dropout's function with (site, row,
 * column) in the places of (head, query row, key row): Philox2x32-10, counter = (row, column >> 2), key = the 32-bit mix of seed and
 * site, one 16-bit field per column of a group of 4, kept when field >= round(p_drop * 65536).  "row" = the row index in the tensors
 * passed to the call.  Stateless: the backward and a recomputed forward evaluate it again.  The caller passes a seed that no
 * attention call of the step uses (ops.bert_hidden_seed).  0 <= p_drop < 1; p_drop < 2^-17 drops nothing and scales nothing.
 * inv_keep = rpo_hidden_dropout_scale(p_drop) = 1 / (1 - p_drop) in f32, the attention kernels' factor.  drop(x) below =
 * round(f32(x) * inv_keep) * keep on a value x of the storage type: the rounding points of a separate dropout pass.
 * bf16 / fp16, d % 8 == 0, d <= 4096, strides % 8 == 0, 16-byte aligned, rows <= 2^31 - 1; rows == 0 does nothing.
 * The three entries launch the DROP = true instances of the row kernels of (9) / (10) (one template per role, the entries of
 * (9) / (10) its DROP = false instances).
 *
 * rpo_add_layernorm_drop_fwd: s = round(a + drop(b)) (b required), y = LayerNorm(s); s stored as rpo_add_layernorm_train_fwd does.
 * rpo_bert_embed_ln_drop_fwd: s as rpo_bert_embed_ln_train_fwd, y = drop(round(LayerNorm(s))).
 * rpo_layernorm_drop_bwd: rpo_layernorm_bwd (the same partials in the same order) with site_in >= 0: dy <- drop(dy) with site_in as
 * it is loaded (the backward of rpo_bert_embed_ln_drop_fwd); db != NULL: db = drop(round(ds)) with site_out written beside ds (the
 * backward of rpo_add_layernorm_drop_fwd: ds is the gradient of a, db that of b).  A negative site switches its side off.
 * rpo_hidden_dropout_mask: mask[i][c] (uint8, 1 = kept) for rows row0 + i < row0 + rows, columns c < d.  Tests and diagnostics only.
 * --------------------------------------------------------------------------------------------- */
float rpo_hidden_dropout_scale(float p_drop);   /* 0 for p_drop outside [0, 1) */
int rpo_add_layernorm_drop_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma, const void* beta,
                               float eps, void* y, int64_t ldy, void* s, int64_t lds, int64_t rows, int64_t d, int dtype,
                               float p_drop, uint64_t seed, int64_t site, rpo_stream_t stream);
int rpo_bert_embed_ln_drop_fwd(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word,
                               int64_t vocab, const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos,
                               const void* gamma, const void* beta, float eps, void* y, int64_t ldy, void* s, int64_t lds,
                               int64_t d, int dtype, float p_drop, uint64_t seed, int64_t site, rpo_stream_t stream);
int rpo_layernorm_drop_bwd(const void* s, int64_t lds, const void* gamma, const void* dy, int64_t lddy, float eps, void* ds,
                           int64_t ldds, void* db, int64_t lddb, float* dgamma_partial, float* dbeta_partial, int64_t rows,
                           int64_t d, int dtype, float p_drop, uint64_t seed, int64_t site_in, int64_t site_out,
                           rpo_stream_t stream);
int rpo_hidden_dropout_mask(int64_t row0, int64_t rows, int64_t d, float p_drop, uint64_t seed, int64_t site,
                            unsigned char* mask, rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (10c) embedding-table gradient of (10) without atomics (rankpo_amd/csrc/embed_grad.hip; opt-in:
 * encoder.BERT_DETERMINISTIC_EMBED_GRAD).  out [table_rows, d] (row stride ldout) receives, for every table row r that occurs in
 * the ids, the sum of the rows t of ds [tokens, d] (row stride ldds) with ids[t] == r; the caller zero-fills out, and rows that do
 * not occur, and row padding_idx (-1: none), are not written.  The ids reach the call as a plan built on the host
 * (ops.embed_grad_plan), int32 on the device:
 *   order  [tokens]        the stable ascending sort of the ids (packed-token indices)
 *   chunks [n_chunks, 4]   (table row, first position in order, rows, slot): every run of equal ids in order (a segment) cut into
 *                          consecutive chunks from its first row; slot = -1 for the only chunk of its segment, else the chunk's
 *                          workspace row: a segment's chunks hold consecutive slots in chunk order
 *   multi  [n_multi, 3]    (table row, first slot, chunks) of every segment with several chunks; n_partials = the slots in all
 * THE ORDER OF THE SUM IS PART OF THE CONTRACT: a chunk's rows are added one after the other in f32, in ascending packed-token
 * order, onto 0; a segment of one chunk is then rounded once to the storage dtype and stored; a segment of several chunks stores
 * its f32 chunk sums to the workspace, and a second launch adds them one after the other in ascending chunk order onto 0 and
 * rounds once.  No atomics; nothing depends on how blocks are scheduled: equal arguments give equal bits.  Inf / NaN in ds reach
 * the (row, column) they belong to and no other.  One wave per (chunk, 512-column slice).
 * bf16 / fp16 (RPO_DT_F32: RPO_ERR_UNSUPPORTED), d % 8 == 0, strides % 8 == 0, 16-byte aligned ds / out / workspace (else
 * RPO_ERR_UNSUPPORTED); tokens, table_rows <= 2^31 - 1.  workspace: f32, at least rpo_embed_grad_workspace_elems(n_partials, d)
 * elements (RPO_ERR_WORKSPACE otherwise; NULL when n_partials == 0).  tokens == 0 does nothing.  A plan entry out of range is
 * skipped (a token index: clamped), never followed outside the buffers.
 * --------------------------------------------------------------------------------------------- */
int64_t rpo_embed_grad_workspace_elems(int64_t n_partials, int64_t d);
int rpo_embed_grad_sorted(const void* ds, int64_t ldds, int64_t tokens, int64_t d, int dtype, const int* order, const int* chunks,
                          int64_t n_chunks, const int* multi, int64_t n_multi, int64_t n_partials, void* out, int64_t ldout,
                          int64_t table_rows, int64_t padding_idx, float* workspace, int64_t workspace_elems,
                          rpo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (8) exact top-k over score rows, merged chunk by chunk ("next" row f3: the k-selection of faiss.IndexFlatIP.search,
 * reference src/utils.py:58-80).  scores: [rows, cols] (row stride ld elements) of the chunk whose first column is corpus
 * row col0; best_val f32 [rows, k] / best_idx int64 [rows, k]: the winners so far, best first (value descending, ties by
 * the smaller corpus index); first != 0: best_* hold nothing yet.  Unfilled slots are (-inf, INT64_MAX).  k <= 1024.
 * --------------------------------------------------------------------------------------------- */
int rpo_topk_merge(const void* scores, int64_t ld, int64_t rows, int64_t cols, int64_t col0, int k, int dtype,
                   float* best_val, int64_t* best_idx, int first, rpo_stream_t stream);
/* The same with `split` winner lists per score row: list r * split + s collects columns [s seg, (s + 1) seg) of row r, seg =
 * ceil(cols / split) rounded up to whole 16-byte vectors; best_val / best_idx: [rows * split, k].  A search of a FEW query rows
 * (256, the reference's faiss_search batch: utils.py:58-80) is one block per list: split = 4 fills the 256 CUs four times over
 * where one list per row leaves each CU one block.  The caller merges the `split` lists of a row once, at the end of the search
 * (value descending, ties by the smaller index: the same order).  split == 1 is rpo_topk_merge. */
int rpo_topk_merge_split(const void* scores, int64_t ld, int64_t rows, int64_t cols, int64_t col0, int k, int dtype, int split,
                         float* best_val, int64_t* best_idx, int first, rpo_stream_t stream);

/* The search step with the k-selection FUSED into the scoring kernel (round 6; bf16 operands -- dtype RPO_DT_BF16 --, d a multiple of 64, both operands below
 * 4 GB): the [Q, P] score matrix of the query block against one corpus chunk (p: rows [col0, col0 + P) of the corpus) is never written.
 * A score -- <q_r, p_c> accumulated in f32, rounded to bf16 once: bit for bit what the eval similarity (rpo_infonce_fwd without
 * temperature) stores -- that beats row r's current k-th winner, (best_val, best_idx)[r k + k - 1] in the order of rpo_topk_merge,
 * is appended to row r's candidate list: slot = atomic increment of cand_cnt[r]; cand_val f32 / cand_idx int64 [Q, cap]; a slot
 * >= cap is dropped (the counter still counts it).  cand_cnt must be zero on entry (rpo_topk_merge_candidates leaves it so).
 * The caller's winners must be FULL (k real entries per row: e.g. the first chunk went through rpo_topk_merge), otherwise every
 * column passes.
 * rpo_topk_merge_candidates: row r's min(cand_cnt[r], cap) candidates + its k winners -> its k winners (same order); resets
 * cand_cnt[r]; sets *overflow = 1 if any list had dropped entries (the caller then redoes the search through the score matrix:
 * retrieval.FlatIPIndex.search).  k + cap <= 4096.
 * rpo_sim_topk_filter_ok(Q, P, d): 1 for the shapes the filter takes -- those rpo_infonce_fwd scores with the same 256 x 256 kernel
 * frame (more than 64 query rows, d % 64 == 0, >= 192 tiles, operands below 4 GB), so that the fused step and the score-matrix path
 * agree bit for bit; everything else returns RPO_ERR_UNSUPPORTED and stays on the score-matrix path. */
int rpo_sim_topk_filter_ok(int64_t Q, int64_t P, int64_t d);
int rpo_sim_topk_filter(const void* q, const void* p, int64_t Q, int64_t P, int64_t d, int dtype, int64_t col0, int k,
                        int round_scores, const float* best_val, const int64_t* best_idx, float* cand_val, int64_t* cand_idx,
                        int32_t* cand_cnt, int cap, rpo_stream_t stream);
/* round_scores = 0 and rpo_sim_scores_f32: the search of an F32 index (the reference's faiss.IndexFlatIP dtype, utils.py:38-51) whose
 * embeddings are exactly representable in bf16 (dtype RPO_DT_BF16) or fp16 (RPO_DT_F16; f32 scores only) -- what an encoder that
 * computes in bf16 / fp16 hands over (modeling.py:533-539).  Products of such values are exact in f32 and the sums are f32 sums: an
 * f32 inner product in this kernel's summation order, at the 16-bit MFMA rate (16 x the f32 MFMA's).  The score is the unrounded
 * f32 sum; rpo_sim_scores_f32 writes the [Q, P] score matrix (row stride ldc floats) of the same frame for the search's first
 * chunk, so that equal rows score equal wherever they lie.  Same shapes as the filter. */
int rpo_sim_scores_f32(const void* q, const void* p, int64_t Q, int64_t P, int64_t d, int dtype, float* scores, int64_t ldc,
                       rpo_stream_t stream);
int rpo_topk_merge_candidates(const float* cand_val, const int64_t* cand_idx, int32_t* cand_cnt, int64_t rows, int cap, int k,
                              float* best_val, int64_t* best_idx, int32_t* overflow, rpo_stream_t stream);

/* The search of an F32 index whose values are exact in NEITHER 16-bit type (an f32 encoder's output, f32-normalised embeddings), on the
 * same 16-bit frame: every finite f32 x is h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) as long as the three
 * planes are normal or zero.  The scoring frame walks the plane pairs (q, corpus) = lh, mm, hl, mh, hm, hh -- smallest terms first --
 * into one f32 accumulator: exact products, f32 sums in this frame's order, 6 K-walks against the f32 MFMA's 16; the pairs ml, lm,
 * ll it leaves out are below (2^-23 + 2^-32) |q_i c_i| per element, the size of the rounding of an f32 multiply.
 * rpo_split_bf16x3: planes bf16 [rows, 3 d] (row stride ldp elements), h | m | l per row, of x f32 [rows, d] (row stride ldx);
 *   d % 64 == 0, ldx % 4 == 0, ldp % 8 == 0, 16-byte aligned.  *inexact (device int32) is set to 1 -- never cleared -- when an
 *   element is not finite, its planes do not add up to it in f32 ((float)h + (float)m + (float)l != x) or a plane is a bf16
 *   subnormal: the caller then keeps the f32 kernel.
 * rpo_sim_planes_ok(Q, P, d): the shapes of rpo_sim_topk_filter_ok applied to d, with the operand limit on the planes
 *   (rows * 3 d * 2 bytes below 4 GB).
 * rpo_sim_scores_f32_planes / rpo_sim_topk_filter_planes: rpo_sim_scores_f32 / rpo_sim_topk_filter(round_scores = 0) with q [Q, 3 d]
 *   and p [P, 3 d] planes (contiguous rows) in place of the bf16 operands; everything else as there. */
int rpo_split_bf16x3(const float* x, int64_t ldx, int64_t rows, int64_t d, void* planes, int64_t ldp, int32_t* inexact,
                     rpo_stream_t stream);
int rpo_sim_planes_ok(int64_t Q, int64_t P, int64_t d);
int rpo_sim_scores_f32_planes(const void* q, const void* p, int64_t Q, int64_t P, int64_t d, float* scores, int64_t ldc,
                              rpo_stream_t stream);
int rpo_sim_topk_filter_planes(const void* q, const void* p, int64_t Q, int64_t P, int64_t d, int64_t col0, int k,
                               const float* best_val, const int64_t* best_idx, float* cand_val, int64_t* cand_idx,
                               int32_t* cand_cnt, int cap, rpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RANKPO_HIP_H */
