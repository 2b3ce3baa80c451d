/* mmfusion.h — C ABI of libmmfusion.so: MI355X (gfx950) kernels for the cross-modal fusion path.
 *
 * The reference (nl1xx/simple-multimodal) is pure Python on stock torch.nn and has no FFI of its
 * own, so this ABI is what the reference-side binding for the fusion path
 * would call; each entry point names the reference arithmetic it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (activations, weights, outputs, saved statistics, workspaces); the library never
 *     allocates, frees or synchronises;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and is safe to capture into a hipGraph: descriptor tables travel by value
 *     in the kernel arguments;
 *   - activations / weights are bf16 (bit pattern of the upper half of an IEEE f32), row-major,
 *     leading dimensions in ELEMENTS; accumulation, softmax and LayerNorm statistics are f32;
 *   - return value: MMF_OK or a negative MMF_E_* code; mmf_last_error() gives the thread-local
 *     message.  No C++ exception crosses the boundary.
 *   - alignment: all base pointers 16-byte aligned; leading dimensions and K multiples of 8
 *     elements; N multiples of 4.  Violations return MMF_E_ALIGN / MMF_E_SHAPE, nothing is launched.
 */
#ifndef MMFUSION_H
#define MMFUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMF_ABI_VERSION 1

enum {
  MMF_OK = 0,
  MMF_E_SHAPE = -1,
  MMF_E_DTYPE = -2,
  MMF_E_ALIGN = -3,
  MMF_E_LAUNCH = -4,
  MMF_E_UNSUPPORTED = -5
};

int mmf_version(void);
const char* mmf_last_error(void);
/* number of compute units of the current device (grid sizing on the host side) */
int mmf_device_cu_count(void);

/* ------------------------------------------------------------------------------------------
 * Grouped GEMM, bf16 in / f32 accumulate on the MFMA units (v_mfma_f32_16x16x32_bf16).
 * Replaces every dense contraction of the path: nn.MultiheadAttention in/out projections
 * (models/fusion_layers.py:188-191,204), the FFN (:195-200,208), and all fusion MLPs
 * (:21-28,124-128,304-327,395-412,471-476), forward, dgrad and wgrad.
 *
 *   layout MMF_GEMM_NT:  C[m][n] = sum_k A[m][k]  * B[n][k]    (y = x W^T, forward)
 *   layout MMF_GEMM_NN:  C[m][n] = sum_k A[m][k]  * B[k][n]    (dx = dy W, dgrad)
 *   layout MMF_GEMM_TN:  C[m][n] = sum_k A[k][m]  * B[k][n]    (dW = dy^T x, wgrad)
 *
 * Epilogue, applied in this order on the f32 accumulator (dropout and alpha: mmf_gemm_grouped_ex):
 *   + bias[n] (MMF_EPI_BIAS) -> relu (MMF_EPI_RELU) -> keep ? v / (1 - p) : 0 (MMF_EPI_DROPOUT)
 *   -> * (aux[m][n] > 0) (MMF_EPI_MASK_AUX) -> * alpha -> + aux[m][n] (MMF_EPI_ADD_AUX)
 *   -> + C_old[m][n] (MMF_EPI_ACCUM, f32 output only)
 * so a residual (ADD_AUX) and an accumulated old C are neither dropped nor scaled.  The dropout mask of element (m, n) of the
 * caller's problem i is the counter hash's keep of index m * N + n (N, not ldc; mod 2^32) in sub-stream i of (*rng_state, site),
 * whichever kernel generation runs the launch and in whatever order it walks the problems (tests/keyed_dropout_ref.py restates it).
 * aux is bf16 with leading dimension ldaux.  Output is bf16 or f32 (out_f32 != 0).
 * One launch covers all problems (<= MMF_GEMM_MAX_PROBLEMS); problems must not alias outputs.
 * ------------------------------------------------------------------------------------------ */
#define MMF_GEMM_MAX_PROBLEMS 48
enum { MMF_GEMM_NT = 0, MMF_GEMM_NN = 1, MMF_GEMM_TN = 2 };
enum {
  MMF_EPI_BIAS = 1,
  MMF_EPI_RELU = 2,
  MMF_EPI_MASK_AUX = 4,
  MMF_EPI_ADD_AUX = 8,
  MMF_EPI_ACCUM = 16,
  /* TN only: additionally `bias[m] += sum_k A[k][m]` (f32 atomics) — the nn.Linear bias gradient
   * (column sums of dy) taken from the A tiles the wgrad kernel stages anyway; `bias` is then an
   * OUTPUT of length M and MMF_EPI_BIAS must not be set. */
  MMF_EPI_COLSUM_A = 32,
  /* mmf_gemm_grouped_ex only: after ReLU, zero each element with probability extra->dropout_p and scale
   * the kept ones by 1/(1-p) (nn.Dropout in training mode, reference models/fusion_layers.py:198);
   * the mask is a stateless hash of (*extra->rng_state, extra->site, problem index, m*N+n). */
  MMF_EPI_DROPOUT = 64,
  /* The ReLU / dropout keep-mask as one bit per element instead of the activation tensor (generation 7 only; ask
   * mmf_gemm_relu_bits_available first: a launch that would go to generation 6 or 2 is refused with MMF_E_UNSUPPORTED).
   * `aux` of each problem points to its bit buffer of mmf_gemm_relu_bits_bytes(M, N) bytes; ldaux is ignored.
   *   MMF_EPI_RELU_BITS  with MMF_EPI_RELU (with or without MMF_EPI_BIAS / MMF_EPI_DROPOUT; bf16 output): the launch also
   *                      WRITES the bits: a bit is 1 exactly when the bf16 value stored to C is > 0 (so 0 for a positive
   *                      accumulator that rounds to zero, for a unit dropout zeroed, for NaN; 1 for +inf).
   *   MMF_EPI_MASK_BITS  instead of MMF_EPI_MASK_AUX: v = bit ? v * alpha : 0, bit-equal to MMF_EPI_MASK_AUX on the
   *                      activation tensor the bits were taken from.
   * Layout, keyed by the problem's own 32 x 32 blocks and nothing of the launch (tile width, walk): the buffer is an array of
   * uint16_t [ceil(M / 32)][ceil(N / 32)][64]; the word of block (bm, bn) at index 32 * h + r holds row 32 * bm + r, and its bit
   * 2 * g + e / 2 + 8 * (e % 2) (g, e in 0..3) is column 32 * bn + 8 * g + 4 * h + e: even columns in the low byte, odd ones in the
   * high byte.  In other words element (m, n) is bit 2 * ((n % 32) / 8) + (n % 4) / 2 + 8 * (n % 2) of word
   * [m / 32][n / 32][32 * ((n / 4) % 2) + m % 32].  Bits of rows >= M or columns >= N of an edge block hold nothing. */
  MMF_EPI_RELU_BITS = 128,
  MMF_EPI_MASK_BITS = 256
};

typedef struct mmf_gemm_problem {
  const void* A;      /* bf16 */
  const void* B;      /* bf16 */
  void* C;            /* bf16 or f32 */
  const float* bias;  /* f32 [N] or NULL (MMF_EPI_COLSUM_A: f32 [M], accumulated into) */
  const void* aux;    /* bf16 [M][ldaux] or NULL */
  int32_t M, N, K;
  int32_t lda, ldb, ldc, ldaux;
} mmf_gemm_problem;

int mmf_gemm_grouped(const mmf_gemm_problem* problems, int num_problems, int layout,
                     int epilogue, int out_f32, void* stream);
/* Extended form: `alpha` multiplies the result after the mask step (before +aux / accumulate) — the
 * 1/(1-p) of a dropout backward: dH = (dY W2) * (h_dropped > 0) * alpha needs no RNG because dropped
 * units are exactly 0 in the saved activations.  rng_state is a DEVICE pointer to the 64-bit dropout
 * state.  extra == NULL behaves like mmf_gemm_grouped. */
typedef struct mmf_gemm_extra {
  float alpha;
  float dropout_p;
  const uint64_t* rng_state;
  uint32_t site;
} mmf_gemm_extra;
int mmf_gemm_grouped_ex(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue,
                        int out_f32, const mmf_gemm_extra* extra, void* stream);
/* bytes of the bit buffer of an M x N problem (MMF_EPI_RELU_BITS / MMF_EPI_MASK_BITS): rows and columns rounded up to 32 */
size_t mmf_gemm_relu_bits_bytes(int M, int N);
/* 1 when mmf_gemm_grouped_ex with exactly these arguments (epilogue holding MMF_EPI_RELU_BITS or MMF_EPI_MASK_BITS) would run on
 * generation 7 under the current kernel selection, else 0; host only, launches nothing.  Callers decide per launch: where it is 0
 * they launch the form without the bits (MMF_EPI_MASK_AUX on the activation tensor). */
int mmf_gemm_relu_bits_available(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue,
                                 int out_f32, const mmf_gemm_extra* extra);

/* Tuning hook: which kernel mmf_gemm_grouped dispatches to.  0 = automatic [default]; 2 = LDS-DMA ring 256x128; 6 = 256x256 on
 * one wave per SIMD with 128x128 wave tiles [gemm6.hip: any K for TN, K % 32 == 0 for NT / NN, no aux epilogue with f32 output];
 * 7 = generation 6 on persistent workgroups (below).  Automatic (gemm.hip auto_impl): 6 when the launch has 256x256 tiles for at
 * least half of the CUs (TN, wgrad) or a quarter of them (NT / NN) and generation 6 takes its shapes, else 2; a launch that
 * gets 6 is promoted to 7 whenever generation 7 takes it, whatever its tile count.  A pinned
 * generation is used for every launch it takes; the others fall back 7 -> 6 -> 2.  Any other value (1 / 3 left in round 3, 4 / 5
 * in round 4) is refused with MMF_E_UNSUPPORTED.  Results are identical up to f32 summation order (and, with a bias, one bf16 ulp
 * between 6 and 7); exists so that A/B timings can be interleaved inside one process.  A process-wide setting, not synchronised
 * between threads. */
int mmf_gemm_select_impl(int impl);
/* the kernel generation the calling thread's last mmf_gemm_grouped[_ex] call dispatched to (profiling labels) */
int mmf_gemm_last_impl(void);
/* Generation 7 (gemm7.hip): generation 6's tile on PERSISTENT workgroups — one per CU, each walking the tiles w, w + grid, ... of
 * the launch with its LDS ring running on across tile boundaries (no ring fill and no idle matrix pipe between tiles).  NT / NN
 * with bf16 output, K % 32 == 0, K >= 160, N and the leading dimensions of C / aux multiples of 8, a 16-byte aligned aux, and the
 * flag sets of the fusion step (alpha != 1 only on the NN ReLU mask, MMF_EPI_MASK_AUX / MMF_EPI_MASK_BITS alone); every other launch
 * falls back to generation 6, then 2.  Without a bias bit-identical to generation 6; with one the accumulators start from the bias, so
 * outputs may differ from generation 6 by one bf16 ulp on a small fraction of the elements.
 * Tile width: 256 x 256 or 256 x 192, per launch.  Automatic: 192 exactly when the launch's makespan — the longest workgroup's
 * sum of K x width over the tiles the persistent walk gives it — is strictly shorter at 192 than at 256.  Both widths give every
 * output element the same MFMA chain: the results are bit-identical between them.
 * mmf_gemm_set_persistent_workgroups(n): grid size of generation 7 (0 = the CU count [default]); a test / tuning hook: with a
 * small n a small problem exercises many tiles per workgroup.
 * mmf_gemm7_set_tile_n(n): tile width of every generation-7 launch (0 = automatic [default], 256, 192); a test / tuning hook.
 * Both hooks are process-wide and not synchronised between threads. */
int mmf_gemm_set_persistent_workgroups(int n);
int mmf_gemm7_set_tile_n(int n);
/* the tile width (256 / 192) of the calling thread's last generation-7 launch */
int mmf_gemm7_last_tile_n(void);
/* the width the automatic rule gives a launch of these problems on `workgroups` persistent workgroups (0 = the grid the launch
 * would get); host only, launches nothing */
int mmf_gemm7_tile_n(const mmf_gemm_problem* problems, int num_problems, int workgroups);

/* K-segment chains (generation 7): C[m][n] = sum over the chain's segments s of sum_k A_s[m][k] B_s[k][n] — ONE GEMM over
 * K = sum K_s whose operand pieces live in different buffers (the input gradient of a tensor that several linears read: A_s the
 * output gradients, B_s the weights).  A tile's segments are consecutive entries of the persistent walk; at a segment boundary the
 * fetch side switches operands as it does between tiles, the accumulators are kept and nothing is stored.  Every output element's
 * MFMA chain is: bias start, then the k-substeps of segment 0, 1, .. in order — bit-identical to mmf_gemm_grouped on one problem
 * whose A is the segments' A side by side and whose B is the segments' B stacked.  No atomics, no K split.
 * Takes: layout MMF_GEMM_NN, bf16 output, epilogue 0, MMF_EPI_BIAS or MMF_EPI_ADD_AUX (the drain's one aux operand), 1..12
 * chains of 1..4 segments, every K_s a multiple of 32 and >= 160, N and every leading dimension a multiple of 8 (lda >= K_s,
 * ldb / ldc / ldaux >= N), 16-byte aligned pointers, a generation-7 selection (mmf_gemm_select_impl 0 or 7).
 * mmf_gemm_chain_available: 1 when mmf_gemm_grouped_chain takes exactly these arguments, else 0; host only, launches nothing
 * (`stream` is ignored).  mmf_gemm_grouped_chain returns MMF_E_SHAPE for everything else.  The tile width is chosen as for a launch
 * of one problem of K = sum K_s per chain; mmf_gemm7_chain_tile_n is mmf_gemm7_tile_n for chains (host only). */
#define MMF_GEMM_CHAIN_MAX_SEGMENTS 4
#define MMF_GEMM_MAX_CHAINS 12
typedef struct mmf_gemm_segment {
  const void* A;      /* bf16 [M][lda], K columns */
  const void* B;      /* bf16 [K][ldb], N columns */
  int32_t K, lda, ldb, reserved;
} mmf_gemm_segment;
typedef struct mmf_gemm_chain {
  void* C;            /* bf16 [M][ldc] */
  const float* bias;  /* f32 [N] (MMF_EPI_BIAS) or NULL */
  const void* aux;    /* bf16 [M][ldaux] (MMF_EPI_ADD_AUX) or NULL */
  int32_t M, N, ldc, ldaux;
  int32_t num_segments, reserved;
  mmf_gemm_segment seg[MMF_GEMM_CHAIN_MAX_SEGMENTS];
} mmf_gemm_chain;
int mmf_gemm_grouped_chain(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue, void* stream);
int mmf_gemm_chain_available(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue, void* stream);
int mmf_gemm7_chain_tile_n(const mmf_gemm_chain* chains, int num_chains, int workgroups);

/* ------------------------------------------------------------------------------------------
 * Skinny-M linear layers (1 <= M <= 64 rows): the (B, d) MLPs of the Early / Contrastive / Adaptive /
 * Graph / meta branches (models/fusion_layers.py:21-28, 304-327, 395-412, 471-476) and MulT's pooled
 * projections.  Weight-streaming MFMA kernels with the weight tile on the MFMA row axis; the grouped GEMM
 * above would spend >90 % of a 256-row tile on padding.
 *   fwd:   Y[m][n] = act(sum_k X[m][k] W[n][k] + bias[n])           flags: MMF_EPI_BIAS | MMF_EPI_RELU
 *   dgrad: Y[m][k] = (sum_n X[m][n] W[n][k]) * (aux[m][k] > 0) * alpha   flags: MMF_EPI_MASK_AUX
 *          (X = dy [M][N], W [N][K], Y = dx [M][K]; N = W rows = reduction, K = W columns)
 * X, W, aux bf16; Y bf16 or f32; wgrad goes through mmf_gemm_grouped (TN).
 * ------------------------------------------------------------------------------------------ */
#define MMF_SKINNY_MAX_PROBLEMS 24
typedef struct mmf_skinny_problem {
  const void* X;      /* bf16 [M][ldx] */
  const void* W;      /* bf16 [N][ldw] */
  void* Y;            /* bf16 or f32 */
  const float* bias;  /* f32 [N] (fwd) or NULL */
  const void* aux;    /* bf16 [M][ldaux] (dgrad mask) or NULL */
  int32_t M, N, K;    /* W is N x K */
  int32_t ldx, ldw, ldy, ldaux;
} mmf_skinny_problem;
int mmf_skinny_linear_fwd(const mmf_skinny_problem* problems, int num_problems, int flags, int out_f32, void* stream);
int mmf_skinny_linear_dgrad(const mmf_skinny_problem* problems, int num_problems, int flags, float alpha, int out_f32,
                            void* stream);
/* the strip width of the calling thread's last dgrad launch (mmf_skinny_linear_dgrad[_ex]): 4, 2 or 1 sixteen-column tiles of K
 * per workgroup (4 when the launch has >= 128 64-column strips in all, 2 from 48, else 1); 0 before any call. */
int mmf_skinny_last_strip(void);
/* Round 4: the launches AROUND a (B, d)-row linear folded into it — these rows cost a launch (~5 us) per kernel, not bandwidth
 * (models/fusion_layers.py:21-28,304-327,395-412,471-476: every Linear there is followed by ReLU and / or Dropout and fed by a cat
 * or a pooled f32 tensor).
 *   forward  X may be f32 (narrowed while loaded); MMF_EPI_DROPOUT: Y = dropout(act(X W^T + b)) with the build's counter-based
 *            masks (element m * N + n of stream `site`, problem i); Y2: a second copy of the output in the OTHER dtype (the bf16
 *            operand of the next linear beside the f32 value the module returns), or NULL; with an f32 X, `dz` (if not NULL)
 *            receives the narrowed input as bf16 [M][lddz] — the weight gradient's other operand.
 *   dgrad    dz = dY * (gate > 0) * gate_scale [* keep / (1 - p) with MMF_EPI_DROPOUT: the mask of the forward with the same site]
 *            is formed while dY (bf16 or f32) is loaded — gate = the forward's saved output (ReLU, or ReLU + dropout whose dropped
 *            units are exactly 0: gate_scale = 1 / (1 - p)) — and dx = dz W; `dz` (bf16, lddz) receives the gated gradient for the
 *            weight-gradient launch.  MMF_EPI_MASK_AUX / alpha act on dx as in mmf_skinny_linear_dgrad. */
typedef struct mmf_skinny_problem_ex {
  mmf_skinny_problem p;
  void* Y2;
  const void* gate;
  void* dz;
  int32_t ldy2, ldgate, lddz, reserved;
} mmf_skinny_problem_ex;
typedef struct mmf_skinny_extra {
  int32_t x_f32;        /* X (forward) / dY (dgrad) is f32 */
  int32_t gate_f32;     /* the gate tensor is f32 */
  float gate_scale;
  float dropout_p;
  const uint64_t* rng_state;
  uint32_t site;
  uint32_t reserved;
} mmf_skinny_extra;
int mmf_skinny_linear_fwd_ex(const mmf_skinny_problem_ex* problems, int num_problems, int flags, int out_f32,
                             const mmf_skinny_extra* extra, void* stream);
int mmf_skinny_linear_dgrad_ex(const mmf_skinny_problem_ex* problems, int num_problems, int flags, float alpha, int out_f32,
                               const mmf_skinny_extra* extra, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-step loss and ModalityDropout as one launch each (round 4; csrc/loss.hip).
 * mmf_fusion_loss: replaces the loss of training/advanced_trainer.py:139-166 —
 *   loss = mean_b CE_ls(logits[b], targets[b]) + sum_j extra_w[j] * extra[j][0]
 * with CE_ls = (1 - eps) * (-log p_y) + eps * (-(1 / C) sum_c log p_c) (torch's label_smoothing), C <= 64 — and writes
 * dlogits[b][c] = d loss / d logits (f32 [B][C], may be NULL).  extra[j]: device scalars (the contrastive / distillation losses).
 * mmf_modality_dropout: replaces models/encoders.py:289-321 — y_m[b] = x_m[b] * keep[b][m] for the three (B, d) f32 feature
 * tensors; draw != 0: keep[b][m] ~ Bernoulli(1 - p) from the counter-based hash of (*rng_state, site, 3 b + m), a sample with no
 * modality left gets one back, the masks are written to `keep` (f32 [B][3]); draw == 0: `keep` is applied as given (backward).
 * ------------------------------------------------------------------------------------------ */
int mmf_fusion_loss(const float* logits, int ldl, const int64_t* targets, int B, int C, float label_smoothing,
                    const float* const* extra, const float* extra_w, int n_extra, float* loss, float* dlogits, void* stream);
int mmf_modality_dropout(const float* const* x, float* const* y, float* keep, int B, int d, float p,
                         const uint64_t* rng_state, uint32_t site, int draw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Knowledge distillation loss (csrc/loss.hip).
 * mmf_distill_kl: replaces models/multimodal_model.py:250-256 —
 *   loss = T^2 * (1 / B) sum_b KL(softmax(teacher[b] / T) || softmax(student[b] / T))   (F.kl_div(..., "batchmean") * T^2)
 * over (B, C <= 64) f32 logits with row strides lds, ldt >= C (the teacher's logits may be a view), B unbounded, and writes
 * dstudent[b][c] = (T / B) (softmax(student[b] / T)_c - softmax(teacher[b] / T)_c) (f32 dense [B][C], may be NULL: value only).
 * The teacher gets no gradient.  A teacher probability that underflows to 0 contributes 0 (torch's xlogy).
 * mmf_fusion_loss_kd: mmf_fusion_loss + kd_weight * mmf_distill_kl(logits, teacher) in ONE launch — the distillation training
 * step's loss (training/advanced_trainer.py:139-166 with its 0.5 x distillation term): value and d/dlogits.
 * Both refuse (MMF_E_SHAPE, nothing launched) a null student / teacher / loss, C outside 1..64, a row stride below C, a
 * temperature that is not finite and > 0; mmf_fusion_loss_kd also everything mmf_fusion_loss refuses and a non-finite kd_weight.
 * ------------------------------------------------------------------------------------------ */
int mmf_distill_kl(const float* student, int lds, const float* teacher, int ldt, int B, int C, float temperature,
                   float* loss, float* dstudent, void* stream);
int mmf_fusion_loss_kd(const float* logits, int ldl, const int64_t* targets, int B, int C, float label_smoothing,
                       const float* const* extra, const float* extra_w, int n_extra,
                       const float* teacher, int ldt, float temperature, float kd_weight,
                       float* loss, float* dlogits, void* stream);

/* ------------------------------------------------------------------------------------------
 * Robust head of RobustMultimodalModel (csrc/small.hip).  Replaces models/multimodal_model.py:404-440 after the
 * predictor's hidden layer h = relu(W1 [f_t; f_a; f_v] + b1) (which stays on the row linear).  Per sample b:
 *   a    = sigmoid(W2 h + b2)                       [B][3]   "modality_availability"
 *   p_m  = W_m f_m + b_m,  m = t, a, v              [B][C]   "individual_predictions"
 *   w    = a (avail = -1), or the constant mask bits of avail in 0..7 (bit 0 text, 1 audio, 2 video; no gradient to a)
 *   wn_m = w_m / ((w_t + w_a + w_v) + 1e-8)         [B][3]   "modality_weights" (f32, the reference's order: a given mask
 *                                                             yields exactly 1, 1/2, 1/3 or 0)
 *   y    = wn_t p_t + wn_a p_a + wn_v p_v           [B][C]   "robust_prediction"
 * f_m, h: f32 dense [B][d]; W2 [3][d], b2 [3], W_m [C][d], b_m [C]: the f32 masters.  Forward: one workgroup per sample.
 * Backward (one launch, no atomics: eager and replayed runs are bit-identical), given g = dL/dy and the optional direct
 * gradients dP_m [B][C], dA [B][3], dN [B][3] (NULL: none; dP itself may be NULL):
 *   dwn_m = g . p_m + dN_m,  dp_m = wn_m g + dP_m
 *   predicted: dz_m = (dA_m + (dwn_m - sum_k wn_k dwn_k) / (S + 1e-8)) a_m (1 - a_m);   given: dz_m = dA_m a_m (1 - a_m)
 *   df_m = W_m^T dp_m, dh = W2^T dz (written; NULL: not needed, df itself may be NULL);
 *   dW_m += dp_m^T f_m, db_m += sum_b dp_m, dW2 += dz^T h, db2 += sum_b dz (accumulated into the gradient arena).
 * a, p_m, wn are the forward's outputs.  Limits: B <= 256 (the backward holds B (3C + 3) floats of per-sample scalars in
 * LDS, <= 51 KiB), C <= 16, d a multiple of 4, features / h / W2 / W_m 16-byte aligned.  Refused, nothing launched:
 * MMF_E_SHAPE for a null operand, output or parameter gradient, B, C or d out of range, avail outside -1..7;
 * MMF_E_ALIGN for a misaligned operand.
 * ------------------------------------------------------------------------------------------ */
int mmf_robust_head_fwd(const float* const f[3], const float* h, const float* W2, const float* b2,
                        const float* const Wm[3], const float* const bm[3], int avail, float* a, float* const p[3],
                        float* wn, float* y, int B, int d, int C, void* stream);
int mmf_robust_head_bwd(const float* const f[3], const float* h, const float* W2, const float* const Wm[3],
                        const float* a, const float* const p[3], const float* wn, int avail, const float* g,
                        const float* const dP[3], const float* dA, const float* dN, float* const df[3], float* dh,
                        float* dW2, float* db2, float* const dWm[3], float* const dbm[3], int B, int d, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Episode head of FewShotModel (csrc/fewshot.hip).  Replaces models/multimodal_model.py:286-362 around the prototype MLP
 * (which stays on the row linear).  Support rows are class-major: row r = c * n_shot + s, S = n_way * n_shot.
 *   proto_fwd:  sf[r] = (t[r] + a[r]) + v[r]               [S][d]      "support_features" (the reference's order)
 *               mean[c] = (sum_s sf[c * n_shot + s]) / n_shot [n_way][d]  summed in shot order, f32
 *   proto_bwd:  ds[r] = dmean[c] / n_shot + dsf[r]           [S][d]      dsf may be NULL; ds is the gradient of t, a and v
 *   dist_fwd:   qf[i] = (t[i] + a[i]) + v[i]                 [Nq][d]     "query_features"
 *               dist[i][j] = sqrt(sum_k (qf[i][k] - P[j][k])^2) [Nq][n_way] direct differences (torch.cdist at these sizes)
 *               pred[i] = softmax(-dist[i])                   [Nq][n_way] accurate expf on max-subtracted values
 *   dist_bwd:   given gdist = dL/ddist and gpred = dL/dpred (either may be NULL: none),
 *               g_ij = gdist_ij - pred_ij (gpred_ij - sum_k pred_ik gpred_ik),  c_ij = g_ij / dist_ij, 0 where dist_ij = 0
 *               (torch's cdist backward: a query on a prototype sends it no gradient);
 *               dq[i] = sum_j c_ij (qf[i] - P[j]),  dp[j] = -sum_i c_ij (qf[i] - P[j])   (written; either may be NULL)
 *               One launch: a workgroup per query row for dq and per prototype for dp, no atomics (bit-deterministic).
 * All tensors f32 dense.  Limits: d a multiple of 4 and <= 1024, 1 <= n_way <= 64, 1 <= n_shot <= 64, 1 <= Nq <= 1024;
 * feature rows, P, dq, dp 16-byte aligned.  Refused, nothing launched: MMF_E_SHAPE for a null required pointer or a size
 * out of range, MMF_E_ALIGN for a misaligned row operand.
 * ------------------------------------------------------------------------------------------ */
int mmf_fewshot_proto_fwd(const float* const s[3], float* sf, float* mean, int n_way, int n_shot, int d, void* stream);
int mmf_fewshot_proto_bwd(const float* dmean, const float* dsf, float* ds, int n_way, int n_shot, int d, void* stream);
int mmf_fewshot_dist_fwd(const float* const q[3], const float* P, float* qf, float* dist, float* pred, int Nq, int n_way,
                         int d, void* stream);
int mmf_fewshot_dist_bwd(const float* qf, const float* P, const float* dist, const float* pred, const float* gdist,
                         const float* gpred, float* dq, float* dp, int Nq, int n_way, int d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics, one launch per batch (csrc/metrics.hip).  Replaces the per-batch tail of training/advanced_trainer.py:
 * 209-263 (validate), :607-660 (evaluate_robustness) and evaluate_model.py:55-203 (evaluate_dataset): CrossEntropyLoss,
 * softmax, argmax and the host copies behind sklearn.  Adds one batch to device-resident accumulators:
 *   counts (int64, n_heads * C * C + 2):  [h][t][p] += #rows of head h with target t and prediction p  (row = target,
 *                                         column = prediction; prediction = argmax with torch's rule: the lowest index
 *                                         among equal maxima, the first NaN if the row holds one);
 *                                         [n_heads C C] += #rows whose target is < 0 or >= C (never used as an index:
 *                                         the caller raises), [n_heads C C + 1] += 1 (the batch count);
 *   sums (f64, MMF_EVAL_NSUMS), head 0 only: [0] += mean_b CE_ls(logits[b], t[b]) (torch's label smoothing, rows with an
 *                                         invalid target adding 0), [1] += sum_b pmax_b, [2] += sum_b pmax_b^2,
 *                                         [3] += sum_b pmax_b over the rows predicted correctly;  pmax_b = max_c softmax_c.
 * logits[h]: f32 (B, C) with row stride ld[h] >= C, h < n_heads <= MMF_EVAL_MAX_HEADS (the main head, then e.g. late
 * fusion's text / audio / video logits); targets int64 (B).  Optional outputs (NULL: not written), rows row0 .. row0 + B - 1
 * of caller buffers with `capacity` rows: pred_out int64 (head 0's argmax), target_out int64 (the targets as given),
 * prob_out f32 dense (capacity, C) (head 0's softmax).  One workgroup, no atomics to global memory: the same inputs give
 * the same bits on every run.  Refused, nothing launched: MMF_E_SHAPE for B <= 0, C outside 1..64, n_heads outside
 * 1..MMF_EVAL_MAX_HEADS, a null operand, a row stride < C, label_smoothing outside [0, 1), output rows beyond capacity;
 * MMF_E_ALIGN for logits / prob_out not 4-byte or targets / counts / sums / pred_out / target_out not 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define MMF_EVAL_MAX_HEADS 4
#define MMF_EVAL_NSUMS 4
int mmf_eval_accumulate(const float* const* logits, const int* ld, int n_heads, const int64_t* targets, int B, int C,
                        float label_smoothing, int64_t* counts, double* sums, int64_t* pred_out, int64_t* target_out,
                        float* prob_out, int64_t row0, int64_t capacity, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grouped fused attention (flash-style: no (Tq,Tk) score matrix in HBM).
 * Replaces q*scale, QK^T, softmax, P.V of F.multi_head_attention_forward as called at
 * models/fusion_layers.py:161-163,204 (six cross blocks + three self blocks of MulT in ONE
 * launch) and models/encoders.py:152-154,236-238.
 * Row r = b*T + t of Q/K/V/O holds head h at columns [h*head_dim, (h+1)*head_dim).
 * head_dim in {64, 96}.  LSE[(b*H + h)*Tq + q] (f32) = ln sum_k exp(scale * q.k): the NATURAL logarithm of the sum over
 * the keys of the exponentials of the SCALED scores (undropped under dropout), written by the forward, read by the backward.
 * Backward recomputes the probabilities p = exp(scale * q.k - LSE).  delta[(b*H + h)*Tq + q] (f32) = sum_c O[q][c] * dO[q][c]
 * over the head's columns, from the bf16 O and dO the backward is given: the dQ kernel writes it and the dK/dV kernel, launched
 * behind it, reads it (dS = p * (dP - delta)); the caller provides the buffer and may read it afterwards.
 * ------------------------------------------------------------------------------------------ */
#define MMF_ATTN_MAX_PROBLEMS 12
typedef struct mmf_attn_problem {
  const void* Q; const void* K; const void* V;   /* bf16 */
  void* O;                                       /* bf16 */
  float* LSE;                                    /* f32 [B*H*Tq] */
  /* backward only (NULL in forward) */
  const void* dO;                                /* bf16, same layout as O */
  float* delta;                                  /* f32 [B*H*Tq], written by the backward (see above) */
  void* dQ; void* dK; void* dV;                  /* bf16, same layouts/strides as Q, K, V */
  int32_t B, H, Tq, Tk;
  int32_t ldq, ldk, ldv, ldo;                    /* row strides (elements) of Q,K,V,O (and grads) */
} mmf_attn_problem;

int mmf_attn_fwd_grouped(const mmf_attn_problem* problems, int num_problems, int head_dim,
                         float scale, void* stream);
int mmf_attn_bwd_grouped(const mmf_attn_problem* problems, int num_problems, int head_dim,
                         float scale, void* stream);
/* The backward's delta by its definition, delta[b][h][i] = sum_j p_ij (dO_i . v_j) with p_ij = exp(scale q_i . k_j - LSE_i), in f32
 * from the bf16 Q / K / V / dO and the forward's LSE (O is not read; dQ / dK / dV may be NULL), and mmf_attn_bwd_grouped with that
 * delta as an INPUT.  mmf_attn_bwd_grouped forms delta = dO . O from the bf16 O, so a row of dS sums to dO . (O - bf16(O)) instead of
 * zero; where dQ / dK are much smaller than |dO| |O| suggests (tokens that have grown alike) that residue is all they hold.  The
 * pair costs one more pass over the keys on the vector units.  These two have no dropout; the _keyed entries below do;
 * mmf_attn_bwd_grouped's validation and codes. */
int mmf_attn_delta_f32(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, void* stream);
int mmf_attn_bwd_grouped_delta(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, void* stream);
/* The backward of an attention whose output is consumed only through its mean over the queries (MulT's self-attentions,
 * models/fusion_layers.py:161-168): every query row of batch row b then has the same output gradient u[b].  Here dO points at
 * that (B, ldo) bf16 matrix, ONE row per batch row (head h at columns [h*head_dim, (h+1)*head_dim), row stride ldo as O's),
 * already divided by Tq and rounded to bf16 as mmf_meanpool_cat_bwd rounds it; every other member as in mmf_attn_bwd_grouped.
 * With u_h the head's columns:  c[k] = V[k,:] . u_h,  delta[q] = O[q,:] . u_h,  dS[q][k] = p[q][k] (c[k] - delta[q]),
 * dQ = scale dS K,  dK = scale dS^T Q,  dV[k,:] = (sum_q p[q][k]) u_h: a streaming kernel writes c into the workspace (f32, f32
 * accumulation, V read once), then a dQ kernel (which forms and writes delta from its O rows, f32) and a dK/dV kernel run without
 * the dO.V^T and P^T.dO products of the general backward.  The results are those of mmf_attn_bwd_grouped given the materialised
 * (B*Tq, ldo) dO, up to rounding.
 * workspace: _workspace_bytes(problems, num_problems) bytes = 4 * sum B*H*Tk, 4-byte aligned, need not be initialised.
 * _available answers 0 — and the caller materialises dO for mmf_attn_bwd_grouped_ex — for a head_dim other than 64 / 96 and for
 * dropout_p != 0 (under dropout dP is no longer the same for every query).  Validation and codes of mmf_attn_bwd_grouped;
 * MMF_E_SHAPE for a missing or short workspace. */
int mmf_attn_bwd_grouped_uniform_available(int head_dim, float dropout_p);
size_t mmf_attn_bwd_grouped_uniform_workspace_bytes(const mmf_attn_problem* problems, int num_problems);
int mmf_attn_bwd_grouped_uniform(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* The same with dO made on the way, for the caller that holds the gradient of the POOLED output: dys[i] (HOST array of device
 * pointers) is problem i's (B, lddy) bf16 gradient of mean_q O (16-byte aligned, lddy a multiple of 8 and >= H*head_dim; column
 * blocks of one wider tensor are fine); the streaming kernel writes dO[b][:] = bf16(dys[i][b][:] / Tq) into the problem's
 * (B, ldo) dO buffer — the one row mmf_meanpool_cat_bwd would write Tq times — and uses it; no launch of its own.  MMF_E_ALIGN
 * for a bad dys / lddy; otherwise as above. */
int mmf_attn_bwd_grouped_pooled(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale,
                                const void* const* dys, int lddy, void* workspace, size_t workspace_bytes, void* stream);
/* Attention-probability dropout with a caller-chosen base of the stream id: the mask of (problem, b, h, q, key) is
 * the counter hash's keep of index q*Tk + key under the key of (*rng_state, site, sub-stream problem * 4096 + stream_base + b*H + h)
 * (mmf_dropout's hash: csrc/mmf_internal.h has the two functions), so a one-problem launch of the
 * items item0 .. of a batch with stream_base = item0 * H draws what a launch of the whole batch draws for them (a backbone's chunks);
 * stream_base = 0 is mmf_attn_fwd_grouped_ex's rule.  One problem: stream_base + B*H <= 2^32; several: <= 4096 each.
 *   _fwd_grouped_keyed        mmf_attn_fwd_grouped_ex's forward: O from the dropped, rescaled probabilities, LSE the undropped one.
 *   _delta_f32_keyed          delta[b][h][i] = sum_j p_ij w_ij (dO_i . v_j), w = keep / (1 - p), p_ij from that LSE: the row term of
 *                             the softmax backward under the mask, in f32 (mmf_attn_delta_f32's kernel with the mask drawn again).
 *   _bwd_grouped_delta_keyed  mmf_attn_bwd_grouped_delta with the mask drawn again in both kernels: dS = p (w dp - delta), dV from w p.
 * dropout_p in [0, 1), quantised to 2^-32 as mmf_dropout's; a threshold of 0 launches the plain kernels (rng_state may then be NULL).
 * rng_state 8-byte aligned.  Validates first and launches nothing on an error. */
int mmf_attn_fwd_grouped_keyed(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, float dropout_p,
                               const uint64_t* rng_state, uint32_t site, uint32_t stream_base, void* stream);
int mmf_attn_delta_f32_keyed(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, float dropout_p,
                             const uint64_t* rng_state, uint32_t site, uint32_t stream_base, void* stream);
int mmf_attn_bwd_grouped_delta_keyed(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, float dropout_p,
                                     const uint64_t* rng_state, uint32_t site, uint32_t stream_base, void* stream);
/* With attention-probability dropout (nn.MultiheadAttention(dropout=p) in training mode): the
 * probabilities are dropped/rescaled before P.V, the softmax normaliser uses the undropped row sums;
 * the backward kernels regenerate the same mask from (*rng_state, site, problem, b, h, q, key): stream id
 * problem * 4096 + b*H + h (problem = the index in `problems`, whatever order the launch works in), element q*Tk + key.
 * A problem with B*H > 4096 would share streams with its successor, so dropout_p > 0 with B*H > 4096 is refused
 * (MMF_E_SHAPE), in the forward and in the backward. */
int mmf_attn_fwd_grouped_ex(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale,
                            float dropout_p, const uint64_t* rng_state, uint32_t site, void* stream);
/* Tuning hook kept for ABI stability: 0 (automatic) and 2 select attention2.hip, the only implementation since round 3
 * (LDS-DMA ring, 128 query rows per workgroup, XCD-aware order); any other value is refused with MMF_E_UNSUPPORTED. */
int mmf_attn_select_impl(int impl);
int mmf_attn_bwd_grouped_ex(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale,
                            float dropout_p, const uint64_t* rng_state, uint32_t site, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension (eps inside the sqrt, biased variance, affine), one
 * wavefront per row, f32 statistics by wave reduction.  Replaces nn.LayerNorm at
 * models/fusion_layers.py:205,209 (the residual add is fused into the producing GEMM's epilogue).
 * Forward saves mean and rstd (f32 [rows]).  Backward writes dx (bf16) and ADDS the
 * per-column sums into dgamma/dbeta (f32 [d], caller zeroes or accumulates; problems of one call
 * must not share dgamma/dbeta).
 * ------------------------------------------------------------------------------------------ */
#define MMF_LN_MAX_PROBLEMS 8
typedef struct mmf_ln_problem {
  const void* x;        /* bf16 [rows][d] */
  void* y;              /* fwd: bf16 out.   bwd: unused */
  const float* gamma;   /* f32 [d] */
  const float* beta;    /* f32 [d] (fwd) */
  float* mean;          /* f32 [rows]: written by fwd, read by bwd */
  float* rstd;
  const void* dy;       /* bwd: bf16 [rows][d] */
  void* dx;             /* bwd: bf16 [rows][d] */
  float* dgamma;        /* bwd: f32 [d], accumulated into (dgamma += column sums) */
  float* dbeta;
  int32_t rows;
} mmf_ln_problem;

int mmf_layernorm_fwd_grouped(const mmf_ln_problem* problems, int num_problems, int d, float eps,
                              void* stream);
/* backward needs an f32 workspace of mmf_layernorm_bwd_workspace_bytes(d) bytes (per-workgroup
 * column partial sums; a second small kernel adds them into dgamma/dbeta — no same-address atomics). */
size_t mmf_layernorm_bwd_workspace_bytes(int d);
int mmf_layernorm_bwd_grouped(const mmf_ln_problem* problems, int num_problems, int d,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The backward with a residual gradient folded in: dx = r + LNbwd(dy), r bf16 [rows][d] handed over in the problem's `y` field
 * (which the plain backward does not read).  The add is in f32 in front of dx's one rounding; r may be dx itself (a pre-LN layer's
 * residual gradient is overwritten by the gradient of the layer's input).  The same kernel bodies, workspace and constraints as
 * mmf_layernorm_bwd_grouped; with r = 0 the results are its bits. */
int mmf_layernorm_bwd_add_grouped(const mmf_ln_problem* problems, int num_problems, int d,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* the form the calling thread's last mmf_layernorm_fwd_grouped / _bwd_grouped call dispatched to (tests assert the form they
 * target): 1-4 = the chunk form ln_*_kernel<NCH> (NCH 512-column chunks per row); 100 + 10 NV + H8 = the lane form
 * ln_*_lane_kernel<NV, H8> (d = 512 NV + 256 H8: 110 / 111 / 101 / 120 for d = 512 / 768 / 256 / 1024); 0 before any call. */
int mmf_layernorm_last_form(void);

/* norm2 of two blocks fused with the three-way sum that consumes them (models/fusion_layers.py:156-158 behind :209):
 *   e = x + LN(pre_a; gamma_a, beta_a) + LN(pre_b; gamma_b, beta_b)
 * in one pass over pre_a, pre_b and x.  Bit-equal to mmf_layernorm_fwd_grouped on (pre_a, pre_b) followed by mmf_add3_grouped on
 * (x, y_a, y_b): each normalised value is rounded to bf16 where the stored tensor would have been, then the sum is formed in f32
 * left to right and rounded once; the statistics are the ones the separate forward writes, and mmf_layernorm_bwd_grouped takes them.
 * The kernel is the lane form (d = 256, 512, 768, 1024; any other d is MMF_E_SHAPE).  The separate forward reduces a row in another
 * order in its chunk form, which it takes for small launches: mmf_layernorm2_add3_available(rows of each sum, num_problems, d) is 1
 * exactly when d is a lane width AND mmf_layernorm_fwd_grouped over the 2 num_problems problems (pre_a, pre_b of every sum) would
 * take the lane form, i.e. when this launch is bit-equal to the two it replaces; where it is 0 the caller composes the two launches.
 * Does not change mmf_layernorm_last_form. */
#define MMF_LN2_ADD3_MAX_PROBLEMS 4
typedef struct mmf_ln2_add3_problem {
  const void* x;          /* bf16 [rows][d] */
  const void* pre_a;      /* bf16 [rows][d] */
  const float* gamma_a;   /* f32 [d] */
  const float* beta_a;
  const void* pre_b;
  const float* gamma_b;
  const float* beta_b;
  void* e;                /* bf16 [rows][d] out */
  float* mean_a;          /* f32 [rows] out */
  float* rstd_a;
  float* mean_b;
  float* rstd_b;
  int32_t rows;
} mmf_ln2_add3_problem;
int mmf_layernorm2_add3_available(const int32_t* rows, int num_problems, int d);
int mmf_layernorm2_add3_fwd_grouped(const mmf_ln2_add3_problem* problems, int num_problems, int d, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Streaming helpers (HBM-bound, 16-byte vector accesses)
 * ------------------------------------------------------------------------------------------ */
/* dst_bf16[i] = bf16(src_f32[i]); n multiple of 8 not required */
int mmf_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int mmf_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* row-strided source (rows x cols, ld_src floats between rows) -> contiguous bf16; cols, ld_src multiples of 4 */
int mmf_cast_f32_to_bf16_2d(const float* src, void* dst, int rows, int cols, int ld_src, void* stream);
/* dst_f32[i] = scale * f32(src_bf16[i]): the receive side of the bf16-compressed gradient all-reduce
 * (mmfusion/dp.py: widen the summed wire buffer and divide by the world size in one pass) */
int mmf_cast_bf16_to_f32_scaled(const void* src, float* dst, int64_t n, float scale, void* stream);
/* y = a + b + c (bf16); models/fusion_layers.py:156-158.  c may be NULL (y = a + b). */
int mmf_add3_bf16(const void* a, const void* b, const void* c, void* y, int64_t n, void* stream);
/* several three-operand sums in one launch (y_i = a_i + b_i + c_i, bf16, n_i elements each) */
#define MMF_ADD3_MAX 8
typedef struct mmf_add3_problem {
  const void* a; const void* b; const void* c;
  void* y;
  int64_t n;
} mmf_add3_problem;
int mmf_add3_grouped(const mmf_add3_problem* problems, int num_problems, void* stream);
/* y = x_0 + ... + x_{n-1} (2 <= n <= MMF_ADDN_MAX bf16 tensors of numel elements, f32 accumulate, bf16 or f32 out) in
 * one pass: the gradient of a tensor the forward used n times (MulT's input rows: models/fusion_layers.py:146-158). */
#define MMF_ADDN_MAX 8
int mmf_addn_bf16(const void* const* xs, int n, void* y, int64_t numel, int out_f32, void* stream);
/* several such sums in one launch (bf16 out): the three modalities' input-gradient sums at the end of MulT's backward were
 * three launches of 6 - 18 us with graph-node gaps between them, alone on the chip in front of the deferred wgrad launch
 * (round 3, profiles/r03_step_timeline.txt) */
#define MMF_ADDN_GROUP_MAX 4
typedef struct mmf_addn_problem {
  const void* x[MMF_ADDN_MAX];
  void* y;
  int64_t numel;
  int32_t n;
} mmf_addn_problem;
int mmf_addn_grouped(const mmf_addn_problem* problems, int num_problems, void* stream);
/* y[b][j] = mean_t x[b][t][j]  (models/fusion_layers.py:166-168); x bf16 [B][T][d], y bf16 with
 * row stride ldy (lets the three pooled modalities land side by side = torch.cat, :171). */
int mmf_meanpool_fwd(const void* x, void* y, int B, int T, int d, int ldy, void* stream);
/* dx[b][t][j] = dy[b][j] / T ; dy bf16 with row stride lddy */
int mmf_meanpool_bwd(const void* dy, void* dx, int B, int T, int d, int lddy, void* stream);
/* the n (<= MMF_POOL_MAX) modalities of :166-171 in one launch: problem i pools xs[i] (B, Ts[i], d) into columns
 * [i d, (i+1) d) of y; backward scatters dy's column blocks back (dxs[i] bf16 (B, Ts[i], d)).  xs / dxs / Ts are
 * HOST arrays. */
#define MMF_POOL_MAX 4
int mmf_meanpool_cat_fwd(const void* const* xs, const int* Ts, int n, void* y, int B, int d, int ldy, void* stream);
int mmf_meanpool_cat_bwd(const void* dy, void* const* dxs, const int* Ts, int n, int B, int d, int lddy, void* stream);
/* out[n] (+)= sum_m x[m][n]; x bf16 [M][ldx]; out f32, atomically accumulated (bias gradients:
 * the column sums of dy for nn.Linear biases).  The grouped form covers several matrices in one launch. */
int mmf_colsum_bf16(const void* x, float* out, int M, int N, int ldx, void* stream);
#define MMF_COLSUM_MAX_PROBLEMS 24
typedef struct mmf_colsum_problem {
  const void* x;      /* bf16 [M][ldx] */
  float* out;         /* f32 [N], accumulated */
  int32_t M, N, ldx;
} mmf_colsum_problem;
int mmf_colsum_grouped(const mmf_colsum_problem* problems, int num_problems, void* stream);
/* y = x * keep / (1-p) elementwise (nn.Dropout, training mode); is_f32 selects f32 or bf16 storage.
 * The same call with the same (*rng_state, site) on dy gives the backward.  In place allowed. */
int mmf_dropout(const void* x, void* y, int64_t n, int is_f32, float p, const uint64_t* rng_state,
                uint32_t site, void* stream);
/* base[starts[r] .. ends[r]) = 0 for up to MMF_ZERO_MAX_RANGES float ranges in ONE launch: the holes of the lazily
 * zeroed gradient arena (biases, LayerNorm vectors, gradients torch produces) between the matrices the wgrad GEMMs
 * overwrite.  base 16-byte aligned; starts / ends are HOST arrays of element offsets. */
#define MMF_ZERO_MAX_RANGES 48
int mmf_zero_ranges_f32(float* base, const int64_t* starts, const int64_t* ends, int n, void* stream);
/* out[i] = (accumulate ? out[i] : 0) + partial[0][i] + partial[1][i] + ... + partial[slabs - 1][i], summed in that order in f32:
 * the K-slab partial products of a weight gradient (slab s at partial + s * n) into the gradient itself.  n % 4 == 0,
 * 1 <= slabs <= MMF_SUM_SLABS_MAX, both pointers 16-byte aligned; no atomics, so two runs give the same bits. */
#define MMF_SUM_SLABS_MAX 64
int mmf_sum_slabs_f32(const float* partial, float* out, int64_t n, int slabs, int accumulate, void* stream);
/* relu backward on bf16: dx = dy * (y > 0) */
int mmf_relu_bwd_bf16(const void* dy, const void* y, void* dx, int64_t n, void* stream);
/* same with dy and / or y in f32 (flags non-zero): narrows and masks in one pass; dx is bf16 */
int mmf_relu_bwd_mixed(const void* dy, int dy_f32, const void* y, int y_f32, void* dx, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small fused kernels of the (B, d)-row branches (csrc/small.hip).  f32 unless said otherwise; every buffer
 * is caller-owned; parameter gradients (datt_*, dbias, dW2, db2, dW, db, demb) are ACCUMULATED into.
 * ------------------------------------------------------------------------------------------ */
/* Dense 3-node GAT layer = torch_geometric GATConv(heads, concat=False) on the directed 3-clique plus self
 * loops, as GraphFusion uses it (models/fusion_layers.py:223-232, 267-282): h [B][3][heads][C] is the node
 * features after the layer's linear map (an mmf_gemm / skinny launch);
 *   e[i,j,h] = leaky_relu(<h[i,h],att_dst[h]> + <h[j,h],att_src[h]>, negative_slope); alpha = softmax_j(e)
 *   (denominator + 1e-16, PyG), dropout(alpha, p); out[i] = mean_h sum_j alpha[i,j,h] h[j,h] + bias
 * y = relu(out) if relu (bf16 [B][3][C], the next layer's GEMM operand); pooled (optional, bf16 [B][C]) = mean over
 * the 3 nodes of y (global_mean_pool, :285-286).  alpha [B][3][3][heads] (before dropout) and sdots [B][2][3][heads]
 * are saved for the backward, which takes dy (bf16 [B][3][C]) and/or dpooled (bf16 [B][C]). */
typedef struct mmf_gat3_params {
  int32_t B, heads, C, relu;
  float negative_slope, dropout_p;
  const uint64_t* rng_state;
  uint32_t site;
} mmf_gat3_params;
int mmf_gat3_dense_fwd(const float* h, const float* att_src, const float* att_dst, const float* bias,
                       void* y_bf16, void* pooled_bf16, float* alpha, float* sdots,
                       const mmf_gat3_params* p, void* stream);
int mmf_gat3_dense_bwd(const float* h, const float* att_src, const float* att_dst, const void* y_bf16,
                       const float* alpha, const float* sdots, const void* dy_bf16, const void* dpooled_bf16,
                       float* dh, float* datt_src, float* datt_dst, float* dbias,
                       const mmf_gat3_params* p, void* stream);
/* n_m = z_m / max(||z_m||, 1e-12) for three (B, D) projections and, if losses != NULL, the symmetric InfoNCE of
 * the pairs (0,1) (0,2) (1,2): (CE(n_a n_b^T / T, arange) + CE(transposed, arange)) / 2 — ContrastiveFusion,
 * models/fusion_layers.py:338-347, 361-375.  B <= 64 (per-rank batch), D a multiple of 4.  inv_norm [3][B] and
 * lse [3][2][B] are saved for the backward; dn[m] / dloss[p] may be NULL (no gradient from that output).  A row whose
 * norm is clamped (||z|| <= 1e-12: a row of zeros) gets a zero gradient row, not dn * 1e12. */
int mmf_infonce_fwd(const float* const z[3], float* const n[3], float* inv_norm, float* losses, float* lse,
                    int B, int D, float temperature, void* stream);
int mmf_infonce_bwd(const float* const n[3], const float* inv_norm, const float* lse, const float* const dn[3],
                    const float* const dloss[3], float* const dz[3], int B, int D, float temperature, void* stream);
/* AdaptiveFusion's weighting (:436-443): aw = softmax(hp W2^T + b2) [B][3]; weighted (bf16 [B][d]) =
 * sum_m attended[b][m][:] aw[b][m].  Backward: dweighted bf16, daw optional. */
int mmf_adaptive_combine_fwd(const float* hp, const float* W2, const float* b2, const float* attended,
                             float* aw, void* weighted_bf16, int B, int d, void* stream);
int mmf_adaptive_combine_bwd(const float* hp, const float* W2, const float* attended, const float* aw,
                             const void* dweighted_bf16, const float* daw, float* dattended, float* dhp,
                             float* dW2, float* db2, int B, int d, void* stream);
/* The head-averaged (B, 3, 3) attention weights AdaptiveFusion returns (:432-434; MultiheadAttention averages its
 * weights over the heads): qkv bf16 [B*3][3 heads head_dim] packed q | k | v.  No gradient (inspection only). */
int mmf_adaptive_attn_weights(const void* qkv_bf16, float* w, int B, int heads, int head_dim, void* stream);
/* The head-averaged (B, T, T) self-attention weights the reference's audio / video encoder heads return
 * (models/encoders.py:152-154,236-238): qkv bf16 [B*T][3 heads head_dim] packed q | k | v; T <= 2048, head_dim % 8 == 0.
 * No gradient (inspection only). */
int mmf_attn_weights_mean(const void* qkv_bf16, float* w, int B, int T, int heads, int head_dim, void* stream);
/* Narrow linear heads, 1 <= N <= 16 outputs, f32 masters (LateFusion :50-60, EmotionClassifier / valence /
 * arousal / uncertainty heads models/multimodal_model.py:56-60,186-219): y = x W^T + b.  dx may be NULL. */
int mmf_linear_narrow_fwd(const float* x, const float* W, const float* b, float* y, int M, int N, int K, void* stream);
int mmf_linear_narrow_bwd(const float* x, const float* W, const float* dy, float* dx, float* dW, float* db,
                          int M, int N, int K, void* stream);
/* x[b][m][:] = feat_m[b][:] + emb[m][:] as bf16 rows (GraphFusion node stacking + type embedding, :255-264;
 * emb == NULL: plain stacking, AdaptiveFusion :427-429).  feat_m rows are ldf floats apart (3d when the three
 * are the thirds of one (B, 3d) buffer).  Backward: any of d0..d2, demb may be NULL; d_m rows ldd apart. */
int mmf_stack3_embed_fwd(const float* f0, const float* f1, const float* f2, const float* emb, void* x_bf16,
                         int B, int d, int ldf, void* stream);
int mmf_stack3_embed_bwd(const void* dx_bf16, float* d0, float* d1, float* d2, float* demb, int B, int d, int ldd,
                         void* stream);
/* y[b][:] = x[b][:] * mask[b]: ModalityDropout's per-sample keep masks (models/encoders.py:289-321, no rescale);
 * the same call on dy is the backward. */
int mmf_rowmask_apply(const float* x, const float* mask, float* y, int B, int d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-step tail on the flat arenas (reference recipe training/advanced_trainer.py:85-110,
 * 168-182: clip_grad_norm_(1.0) then AdamW).  out[0] += sum x^2 ;  AdamW with decoupled weight
 * decay, optional global-norm clipping from the device scalar gnorm_sq (NULL or hparams[7] <= 0:
 * none) and a gradient scale, updating the fp32 masters AND the bf16 shadow in one pass.
 * hparams is a DEVICE array of 9 floats: lr, beta1, beta2, eps, weight_decay, 1-beta1^t,
 * 1-beta2^t, max_grad_norm, grad_scale (device-resident so a captured graph can be replayed with
 * new values).
 * ------------------------------------------------------------------------------------------ */
int mmf_sqnorm_f32(const float* x, int64_t n, float* out, void* stream);
/* Device-side schedule (graph-capturable): *step += 1, then — for sched[0] == 1 — hparams[0] = the OneCycleLR(cos)
 * learning rate of optimiser step (*step - 1) and, for sched[6] != 0, hparams[1] = the cycled beta1 (OneCycleLR's
 * cycle_momentum, on by default and therefore part of the reference recipe, training/advanced_trainer.py:102-110);
 * finally hparams[5], [6] = 1 - beta^step from the current betas, as torch.optim.Adam forms them.
 * sched = {mode, max_lr, total_steps, pct_start, div_factor, final_div_factor, cycle_momentum, base_momentum,
 * max_momentum} as 9 doubles on the device; mode 0 leaves hparams[0], [1] alone. */
int mmf_adamw_advance(int64_t* step, float* hparams, const double* sched, void* stream);
int mmf_adamw_step(float* master, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                   int64_t n, const float* hparams, const float* gnorm_sq, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32-storage parity mode (BASELINE.json north_star: "within 1e-3 fp32").  Every operand f32 in HBM, the exact f32
 * MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fmaf chain) instead of bf16 MFMA.  Same problem struct, layouts
 * and epilogue contract as mmf_gemm_grouped (A, B, C, aux are f32 here; MMF_EPI_DROPOUT is not available).
 * mmf_gemm_f32_batched runs ONE problem over an nb0 x nb1 batch: operand X of batch (i0, i1) starts at
 * X + i0 * strideX[0] + i1 * strideX[1] (elements) — the per-(batch, head) products of the explicit-scores attention
 * the reference computes (torch F.multi_head_attention_forward, need_weights path): S = Q K^T, softmax rows,
 * O = P V, and their backward products.  mmf_softmax_rows_f32: S <- softmax(scale * S) per row, in place;
 * mmf_softmax_bwd_rows_f32: dP <- scale * P * (dP - rowsum(dP * P)), in place.  mmf_layernorm_f32_*: nn.LayerNorm
 * with f32 rows (dgamma / dbeta are accumulated into with atomics).
 * ------------------------------------------------------------------------------------------ */
int mmf_gemm_f32_grouped(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue, float alpha,
                         void* stream);
int mmf_gemm_f32_batched(const mmf_gemm_problem* problem, int layout, int epilogue, float alpha, int nb0, int nb1,
                         const int64_t strideA[2], const int64_t strideB[2], const int64_t strideC[2], void* stream);
int mmf_softmax_rows_f32(float* S, int64_t rows, int cols, float scale, void* stream);
int mmf_softmax_bwd_rows_f32(const float* P, float* dP, int64_t rows, int cols, float scale, void* stream);
int mmf_layernorm_f32_fwd(const float* x, float* y, const float* gamma, const float* beta, float* mean, float* rstd,
                          int rows, int d, float eps, void* stream);
int mmf_layernorm_f32_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd,
                          float* dx, float* dgamma, float* dbeta, int rows, int d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bidirectional LSTM layer recurrence (replaces the per-time-step loop of torch.nn.LSTM / MIOpen behind
 * reference models/encoders.py:183-190,233: nn.LSTM(768, 384, num_layers=2, batch_first=True, bidirectional=True)).
 * The input projections of all time steps are the caller's grouped GEMM (gx); this entry point runs the T sequential
 * steps of both directions in ONE persistent launch with W_hh resident in registers (csrc/lstm.hip), and its backward
 * produces the gate pre-activation gradients dgates that the caller feeds to the grouped dgrad / wgrad GEMMs.
 * Time-major layout: row t*B + b.  Gate order i, f, g, o (torch).  Columns of the 2*4H-wide buffers:
 * [direction 0 | direction 1] x [gate] x [H]; of the 2H-wide buffers: [direction 0 H | direction 1 H].
 * y has a zero row block of B rows in front of time 0 and behind time T-1 (the caller zeroes them once): time t lives in
 * row block t + 1.  B <= 64 per call; H (hidden size per direction) in {64, 128, 384}.
 * workspace: >= mmf_bilstm_workspace_bytes() bytes of device memory, 4-byte aligned; zeroed by the call (stream-ordered);
 * after the launch int32 word [2] is 0, or 1 if a workgroup gave up waiting for its peers (results then invalid).
 * ------------------------------------------------------------------------------------------ */
typedef struct mmf_bilstm_args {
  const void* gx;          /* fwd: f32 (T*B, 2*4H)  x_t W_ih^T, no bias                                        */
  const void* w_hh[2];     /* bf16 (4H, H) per direction                                                      */
  const float* b_ih[2];    /* fwd: f32 (4H)                                                                   */
  const float* b_hh[2];    /* fwd: f32 (4H)                                                                   */
  void* y;                 /* fwd out: bf16 ((T+2)*B, 2H), h_t of time t in row block t+1                      */
  float* gates;            /* fwd out / bwd in: f32 (T*B, 2*4H) gate activations                               */
  float* cell;             /* fwd out / bwd in: f32 (T*B, 2H) cell state c_t                                   */
  const void* dy;          /* bwd in: bf16 (T*B, 2H) gradient of the layer output                              */
  void* dgates;            /* bwd out: bf16 (T*B, 2*4H) gradient of the gate pre-activations                   */
  int32_t T, B, H;
} mmf_bilstm_args;
size_t mmf_bilstm_workspace_bytes(void);
int mmf_bilstm_layer_fwd(const mmf_bilstm_args* args, void* workspace, size_t workspace_bytes, void* stream);
int mmf_bilstm_layer_bwd(const mmf_bilstm_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* out[(i1 * n0 + i0) * d + :] = in[(i0 * n1 + i1) * d + :]  — swaps the two leading axes of an (n0, n1, d) tensor
 * ((B, T, d) <-> (T, B, d)); in_f32 selects an f32 source, the destination is bf16 unless out_f32. d % 8 == 0. */
int mmf_swap01(const void* in, void* out, int n0, int n1, int d, int in_f32, int out_f32, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frozen ViT backbone (mmfusion/vit.py; the reference runs HuggingFace's ViTModel at models/encoders.py:179,216-226).
 * The linears, the attention and the LayerNorms of a ViT layer are the grouped kernels above; these are the three
 * streaming pieces a ViT has beside them.  All pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
/* pixels (N, C, H, W) f32 -> patches (N * (H/P) * (W/P), C*P*P) bf16, row = (n, gy, gx), column = (c, py, px): the A operand of
 * ONE NT GEMM against the Conv2d(C, hidden, P, stride P) weight viewed as (hidden, C*P*P).  H % P == 0, W % P == 0, P % 8 == 0,
 * N <= 65535; anything else is MMF_E_UNSUPPORTED. */
int mmf_vit_patchify(const float* pixels, void* patches_bf16, int N, int C, int H, int W, int P, void* stream);
/* tokens (N*T, d) bf16: row n*T = cls + pos[0], row n*T + 1 + p = patch_emb[n*(T-1) + p] + pos[1 + p]; cls f32 [d], pos f32
 * [T][d], patch_emb bf16 (N*(T-1), d); the add is f32 with one rounding to bf16.  d % 8 == 0, N <= 65535. */
int mmf_vit_embed_tokens(const void* patch_emb_bf16, const float* cls, const float* pos, void* tokens_bf16, int N, int T, int d,
                         void* stream);
/* Its backward, for the gradient g (N*T, d) bf16 of the tokens: dcls[c] += sum_n g[n*T][c]; dpos[t][c] += sum_n g[n*T + t][c]
 * (both f32, summed over n = 0 .. N-1 in that order by one thread per element: no atomics, two runs give the same bits; the sums
 * are ADDED to what the buffers hold); dpatch_emb (N*(T-1), d) bf16 = the rows 1 .. T-1 of every image (the A operand of the patch
 * projection's weight gradient).  mmf_vit_embed_tokens's constraints; validates first and launches nothing on an error. */
int mmf_vit_embed_tokens_bwd(const void* dtokens_bf16, float* dcls, float* dpos, void* dpatch_emb_bf16, int N, int T, int d,
                             void* stream);
/* The attention backward of the CLS route's last layer: one query per image, row 0 of its T rows, on the fused rows q | k | v
 * (N*T, 3 H head_dim) bf16; dout (N, H head_dim) bf16 = the gradient of that query's attention output.  dqkv, laid out as qkv:
 * dq into the q columns of row 0 of each image (the q columns of the other rows are not written), dk | dv into the k | v columns
 * of every row, each rounded to bf16 once.  The softmax is formed again in f32 from the scores and delta = sum_j p_j dp_j, so
 * a row of dS sums to zero up to f32 rounding (mmf_attn_bwd_grouped's delta = dO . O carries the rounding of the bf16 O, which one
 * query's dq and dk do not average out).  Fixed-order sums: two runs give the same bits.  head_dim 64 or 96, T <= 4096,
 * N, H <= 65535; validates first and launches nothing on an error. */
int mmf_vit_cls_attn_bwd(const void* qkv_bf16, const void* dout_bf16, void* dqkv_bf16, int N, int H, int T, int head_dim, float scale,
                         void* stream);
/* x <- gelu(x + bias) in place on a bf16 (rows, cols) block with row stride ld: the exact form v Phi(v) in f32
 * (HuggingFace hidden_act = "gelu"; Phi through erfc, so the left tail keeps its digits), one rounding to bf16.  bias f32 [cols] or NULL.  cols % 8 == 0, ld % 8 == 0. */
int mmf_bias_gelu_bf16(void* x_bf16, const float* bias, int64_t rows, int cols, int ld, void* stream);
/* The out-of-place form: g <- gelu(h + bias) with h kept (a backward reads it); the same kernel body, so g is bit-identical to
 * what the in-place entry leaves in x.  h and g share the row stride ld; mmf_bias_gelu_bf16's constraints. */
int mmf_bias_gelu_bf16_to(const void* h_bf16, const float* bias, void* g_bf16, int64_t rows, int cols, int ld, void* stream);
/* Its backward: dh <- dg * (Phi(v) + v phi(v)), v = h + bias in f32 (h = the stored linear output BEFORE its bias, Phi / phi the
 * standard normal's distribution / density), one rounding to bf16.  dh may be dg.  All three blocks are (rows, cols) bf16 with
 * row stride ld; mmf_bias_gelu_bf16's constraints. */
int mmf_bias_gelu_bwd_bf16(const void* dg_bf16, const void* h_bf16, const float* bias, void* dh_bf16, int64_t rows, int cols, int ld,
                           void* stream);
/* The two with dropout of the GELU's output (Wav2Vec2's activation_dropout).  The rows are `items` items of rows / items rows each;
 * element (t, j) of item g is keyed as mmf_hidden_dropout keys it, sub-stream item0 + g and index t * cols + j, c = 1 / (1 - p):
 *   _drop_bf16_to   g <- keep ? gelu(h + bias) c : 0 in f32, one rounding; h kept raw
 *   _drop_bwd_bf16  dh <- keep ? dg c gelu'(h + bias) : 0, one rounding; dh may be dg
 * bias is required; p in [0, 1) quantised as mmf_dropout's, a threshold of 0 runs the plain kernels (the same bits); rows % items == 0,
 * an item at most 2^32 elements, rows * cols / 8 < 2^31; rng_state 8-byte aligned, the blocks as mmf_bias_gelu_bf16's.  Validates first. */
int mmf_bias_gelu_drop_bf16_to(const void* h_bf16, const float* bias, void* g_bf16, int64_t rows, int cols, int ld, int64_t items, float p,
                               const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream);
int mmf_bias_gelu_drop_bwd_bf16(const void* dg_bf16, const void* h_bf16, const float* bias, void* dh_bf16, int64_t rows, int cols, int ld,
                                int64_t items, float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream);

/* ------------------------------------------------------------------------------------------
 * Wav2Vec2 backbone (mmfusion/wav2vec2.py; the reference runs HuggingFace's Wav2Vec2Model at models/encoders.py:116,144).
 * Activations are channel-last (time, channels) bf16.  The inner feature-extractor convolutions, the projection and the
 * transformer layers are the grouped kernels above; these are the pieces a Wav2Vec2 has beside them.  Every function
 * validates first and launches nothing on an error.
 * ------------------------------------------------------------------------------------------ */
#define MMF_W2V_STATS_SLOTS 128
/* Layer 0, pass 1: Conv1d(1 -> C0, k0, stride s0, no bias) of wave (N, L) f32 against weight (C0, k0) f32, recomputed and
 * reduced (Welford per lane, merged in a fixed order: deterministic) to stats (N, 2, C0) f32: row 0 the mean, row 1 the biased
 * variance over the T0 = (L - k0) / s0 + 1 frames of each (clip, channel).  partial: N * MMF_W2V_STATS_SLOTS * 2 * C0 floats of
 * scratch.  C0 % 8 == 0, C0 <= 2048, k0 <= 16, N <= 65535; stats / partial 16-byte aligned. */
int mmf_w2v_conv0_stats(const float* wave, const float* weight, float* stats, float* partial, int N, int L, int C0, int k0, int s0,
                        void* stream);
/* Layer 0, pass 2: the same convolution recomputed, GroupNorm with one group per channel (stats, gamma, beta f32 [C0], eps),
 * exact GELU, one rounding to bf16, stored in the window form of the NEXT conv layer (kernel k1, stride s1):
 * out (N, T1, k1*C0) bf16 with out[n][t][j*C0 + c] = frame s1*t + j, T1 = (T0 - k1) / s1 + 1. */
int mmf_w2v_conv0_norm_gelu(const float* wave, const float* weight, const float* stats, const float* gamma, const float* beta,
                            void* out_bf16, int N, int L, int C0, int k0, int s0, int k1, int s1, float eps, void* stream);
/* x (N, T_in, C) bf16, a raw convolution output -> out (N, T_out, k*C) bf16, out[n][t][j*C + c] = gelu(x[n][s*t + j][c]) (exact
 * form, f32, one rounding), T_out = (T_in - k) / s + 1: the A operand of the next conv layer as ONE NT GEMM against its weight
 * repacked to (C_out, k*C), column (j, c).  C % 8 == 0, N <= 65535, out must not be x. */
int mmf_w2v_gelu_window(const void* x_bf16, void* out_bf16, int N, int T_in, int C, int k, int s, void* stream);
/* The layer-norm family (feat_extract_norm "layer": large-lv60, XLS-R), whose conv layers are Conv1d(bias) -> LayerNorm over the
 * channels of every frame (gamma, beta f32 [C], eps) -> GELU.  The C / 8 lanes that own a frame reduce its statistics among
 * themselves in f32: the mean, then the squared deviations from it over the values held in registers (never E[x^2] - mean^2);
 * through LDS where a frame spans more than one wave (C > 512).  C / 8 must be a power of two up to 256 (8 .. 2048 channels);
 * no atomics, the same bits on every run.
 *   mmf_w2v_conv0_ln_gelu   layer 0 in one pass: conv0(wave) + bias (NULL: none), LayerNorm, GELU, one rounding, stored in the
 *                           window form of the next layer exactly as mmf_w2v_conv0_norm_gelu stores it.  No statistics pass and
 *                           no stored intermediate.  Its limits (k0 <= 16, N <= 65535) and k1 >= s1; out 16-byte aligned.
 *   mmf_w2v_ln_gelu_window  x (N, T_in, C) bf16, a raw convolution output with its bias added ->
 *                           out[n][t][j*C + c] = bf16(gelu(LN(x[n][s*t + j])[c])), (N, T_out, k*C).  It walks the INPUT rows: a row is
 *                           normalised once and stored to every (t, j) that reads it; rows no window reads are skipped.
 *                           k == 0: the last layer's form, out (N, T_in, C), which may be x.  k >= s otherwise, and out must not be
 *                           x; N <= 65535; x / out 16-byte aligned.
 * MMF_E_SHAPE for null / non-positive / too short operands, MMF_E_UNSUPPORTED for a channel count, k < s or aliasing outside the
 * above, MMF_E_ALIGN for alignment; nothing is launched on an error. */
int mmf_w2v_conv0_ln_gelu(const float* wave, const float* weight, const float* bias, const float* gamma, const float* beta,
                          void* out_bf16, int N, int L, int C0, int k0, int s0, int k1, int s1, float eps, void* stream);
int mmf_w2v_ln_gelu_window(const void* x_bf16, const float* gamma, const float* beta, void* out_bf16, int N, int T_in, int C, int k,
                           int s, float eps, void* stream);
/* Its mirror, the backward of GELU + window form: dwin (N, T_out, k*C) bf16, the gradient of the window form, and the raw x
 * (N, T_in, C) bf16 -> dx (N, T_in, C) bf16,
 *   dx[n][f][c] = gelu'(x[n][f][c]) * sum_{j < k, (f - j) % s == 0, 0 <= (f - j) / s < T_out} dwin[n][(f - j) / s][j*C + c],
 * a gather (each lane owns 8 channels of one frame of dx), the sum in f32 in tap order, one rounding.  Frames no window reads
 * (past s*(T_out - 1) + k - 1) are written as zeros.  C % 8 == 0, k >= s >= 1, N <= 65535; dx may be x, dwin neither. */
int mmf_w2v_window_fold_gelu_bwd(const void* dwin_bf16, const void* x_bf16, void* dx_bf16, int N, int T_in, int C, int k, int s,
                                 void* stream);
/* Layer 0's backward, two passes that recompute c = conv0(wave) as the forward's do and fold dwin1 (N, T1, k1*C0) bf16, the
 * gradient of mmf_w2v_conv0_norm_gelu's output, themselves: with xhat = (c - mean) rstd, y = gamma xhat + beta (stats: the
 * forward's), da0 = the fold of dwin1 (zero on the frames layer 1 never reads) and dy = da0 gelu'(y), all f32:
 *   _bwd_stats  sums (N, 2, C0) f32 = S1 = sum_t dy | S2 = sum_t dy xhat per (clip, channel), summed per frame lane and merged in
 *               slot order; then dbeta (+)= sum_n S1 and dgamma (+)= sum_n S2 in clip order (f32 [C0]).
 *               partial: N * MMF_W2V_STATS_SLOTS * 2 * C0 floats of scratch.
 *   _bwd_wgrad  dc = gamma rstd (dy - S1 / T0 - xhat S2 / T0) on ALL T0 frames (one that layer 1 never reads has dy = 0 but took
 *               part in the statistics); dweight (C0, k0) f32 (+)= sum_{n, t} dc[n][t][ch] wave[n][s0 t + j], through per-lane
 *               partials (clip-major, then slot) added in a fixed tree.  partial: N * MMF_W2V_STATS_SLOTS * C0 * k0 floats of scratch.
 * accumulate != 0 adds to the outputs, 0 overwrites them.  No atomics: the same bits on every run.  The limits of
 * mmf_w2v_conv0_norm_gelu; stats / sums / partial 16-byte aligned. */
int mmf_w2v_conv0_bwd_stats(const float* wave, const float* weight, const float* stats, const float* gamma, const float* beta,
                            const void* dwin1_bf16, float* sums, float* partial, float* dgamma, float* dbeta, int N, int L, int C0,
                            int k0, int s0, int k1, int s1, float eps, int accumulate, void* stream);
int mmf_w2v_conv0_bwd_wgrad(const float* wave, const float* weight, const float* stats, const float* gamma, const float* beta,
                            const void* dwin1_bf16, const float* sums, float* partial, float* dweight, int N, int L, int C0, int k0,
                            int s0, int k1, int s1, float eps, int accumulate, void* stream);
/* The positional convolution with its residual: y = x + gelu(conv(x) + bias), x / y (N, T, C) bf16, Conv1d(C -> C, kernel k,
 * padding k/2, `groups` groups; for an even k the extra last frame is dropped) on the MFMA units with f32 accumulation.
 * w_bf16: (groups, cg, Kp) with cg = C / groups, Kp = k*cg rounded up to a multiple of 32, w[g][co][j*cg + ci] = the
 * convolution weight [g*cg + co][ci][j] and zeros in the padding columns.  bias f32 [C].  cg in {16, 32, 48, 64},
 * (127 cg + Kp) * 2 <= 65536 bytes of LDS, N and groups <= 65535, y must not be x. */
int mmf_w2v_posconv(const void* x_bf16, const void* w_bf16, const float* bias, void* y_bf16, int N, int T, int C, int groups, int k,
                    void* stream);
/* The backward of mmf_w2v_posconv (fine-tuning the front end, mmfusion/wav2vec2.py).  Shapes, the packed weight and the limits are
 * the forward's; the refusals too (MMF_E_SHAPE for a null operand or a size out of range, MMF_E_UNSUPPORTED for a group width, a
 * count or an LDS need beyond the kernel's forms, MMF_E_ALIGN for a pointer that is not 16-byte aligned), and nothing is launched.
 *
 * bwd_act: dz = dy * gelu'(conv(x) + bias), bf16, one rounding.  The pre-activation is computed again by the forward's MFMA loop,
 * not read from memory.  dz must not be x; it may be dy. */
int mmf_w2v_posconv_bwd_act(const void* x_bf16, const void* w_bf16, const float* bias, const void* dy_bf16, void* dz_bf16, int N, int T,
                            int C, int groups, int k, void* stream);
/* dgrad: dx = dy + conv^T(dz): dx[t][g*cg + ci] = dy[t][g*cg + ci] + sum_{j, co} wt[g][ci][j*cg + co] * dz[t + j - (k - 1 - k/2)][g*cg + co],
 * the residual's gradient included.  wt_bf16 (groups, cg, Kp): the forward's weight with the taps reversed and co / ci swapped,
 * wt[g][ci][j*cg + co] = the convolution weight [g*cg + co][ci][k - 1 - j].  The forward's kernel body with k - 1 - k/2 rows of
 * padding in front (k/2 for an odd k).  dx must not be dz; it may be dy. */
int mmf_w2v_posconv_dgrad(const void* dz_bf16, const void* wt_bf16, const void* dy_bf16, void* dx_bf16, int N, int T, int C, int groups,
                          int k, void* stream);
/* wgrad: dw[g*cg + co][j*cg + ci] (+)= sum over clips n and frames t of dz[n][t][g*cg + co] * x[n][t + j - k/2][g*cg + ci], rows
 * outside [0, T) read as zero: f32 in the forward's packed (C, Kp) layout, the padding columns written as zeros.  An MFMA GEMM per
 * (group, 8 taps) whose contraction runs over time; no atomics, the same bits on every run.  slabs == 1: dw (C, Kp) is written
 * (accumulate == 0) or added to.  slabs > 1 (accumulate must be 0): the N * ceil(T / 128) (clip, time block) units are cut into
 * `slabs` runs and dw is (slabs, C, Kp), one partial per run, for mmf_sum_slabs_f32.  slabs <= min(units, MMF_SUM_SLABS_MAX). */
int mmf_w2v_posconv_wgrad(const void* dz_bf16, const void* x_bf16, float* dw, int N, int T, int C, int groups, int k, int slabs,
                          int accumulate, void* stream);
/* The weight norm's backward (weight_norm(dim = 2): w_eff[c][ci][j] = g[j] v[c][ci][j] / ||v[:, :, j]||): from dw (C, Kp) f32, the
 * packed gradient of w_eff, dg[j] += sum dw u and dv (=, with overwrite_v, or +=) (g[j] / ||v_j||) (dw - u dg_j), u = v / ||v_j||.
 * g / dg f32 [k], v / dv f32 (C, cg, k).  One workgroup per tap, f32, fixed reduction order.  C % cg == 0, C cg k < 2^31. */
int mmf_w2v_weightnorm_bwd(const float* dw, const float* g, const float* v, float* dg, float* dv, int C, int cg, int k, int overwrite_v,
                           void* stream);
/* SpecAugment's time mask (HuggingFace _compute_mask_indices without an attention mask), one small launch: starts (N, S_max) int32 =
 * each clip's span starts, -1 in unused slots.  Clip c draws from the hash key of (*rng_state, site, sub-stream item0 + c), draw n =
 * mix32[key + n * 0x9E3779B9] (the keep hash before its threshold):  the count is n0 + (draw 0 >= up), n0 = floor(e), up = ceil((1 - frac(e)) 2^32), e = mask_prob T /
 * length in double (the integer form of int(e + u), u uniform), raised to min_masks, T / length where count * length > T, at most
 * T - (length - 1);  the starts are draws 1, 2, .. as (draw * (T - length + 1)) >> 32, a start already taken drawn again, at most 64
 * draws per start, after which it is the next free value above the last draw, cyclically.  Spans may overlap.  1 <= length <= T,
 * mask_prob in (0, 1], S_max at least the count of n0 + 1.  Validates first and launches nothing on an error. */
int mmf_w2v_mask_spans(int* starts, int N, int S_max, int T, double mask_prob, int length, int min_masks, const uint64_t* rng_state,
                       uint32_t site, int64_t item0, void* stream);
/* Masking and feature-projection dropout in one pass over `items` clips of (T, d) bf16: a row t with starts[g][k] <= t < starts[g][k] +
 * length for some k becomes bf16(embed) (embed f32 [d]; NULL: zeros, the gradient form: dproj = in_span ? 0 : dx0 keep c), any other
 * row is keep ? x c : 0 with the mask of element (t, j) of clip g keyed as mmf_hidden_dropout's: sub-stream item0 + g, index t d + j.
 * starts: the span rows of the call's first clip on, or NULL (dropout only); p = 0: masking only; out may be x.  d % 8 == 0,
 * T d <= 2^32, x / out 16-byte aligned. */
int mmf_w2v_mask_drop(const void* x_bf16, const float* embed, const int* starts, void* out_bf16, int64_t items, int T, int d, int S_max,
                      int length, float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream);
/* The gradient of the mask embedding, first half: partial (slabs, d) f32, partial[s][j] = the sum of dx[r][j] over the rows r of
 * slab s (ceil(rows / slabs) rows each, rows = items * T) that lie inside a span, added in row order.  mmf_sum_slabs_f32 adds the
 * slabs in order: no atomics, the same bits on every run.  1 <= slabs <= min(rows, MMF_SUM_SLABS_MAX). */
int mmf_w2v_mask_embed_grad(const void* dx_bf16, const int* starts, float* partial, int64_t items, int T, int d, int S_max, int length,
                            int slabs, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frozen DeBERTa-v3 backbone (mmfusion/deberta.py; the reference runs HuggingFace's DebertaV2Model at models/encoders.py:20).
 * The linears, the LayerNorms and the MLP of a layer are the grouped kernels above; these are the pieces a DeBERTa has
 * beside them, forward and backward (with respect to the inputs: prompt tuning through the frozen layers; to the position tables:
 * fine-tuning the layers; to the embedding tables and their LayerNorms: full fine-tuning).  All validate
 * first and launch nothing on an error.  A mask is (n, T) as f32 (mask_kind 1, nonzero = keep) or
 * u8 (mask_kind 2), or NULL with mask_kind 0 for all ones.
 * ------------------------------------------------------------------------------------------ */
/* rows of table[ids[row]] (ids int64 [rows], table f32 (vocab, d); an id outside the table reads its nearest row) or, with
 * ids NULL, of embeds f32 (rows, d) -> LayerNorm(gamma, beta, eps) in f32 -> * mask[row] -> out (rows, d) bf16, one rounding.
 * Exactly one of ids / embeds.  d % 4 == 0, d <= 1024; table / embeds / gamma / beta / out 16-byte aligned. */
int mmf_deberta_embed(const int64_t* ids, const float* embeds, const float* table, const float* gamma, const float* beta, float eps,
                      const void* mask, int mask_kind, void* out_bf16, int64_t rows, int d, int vocab, void* stream);
/* Disentangled self-attention forward for head_dim 64, H heads, n items of T tokens:
 *   s[i][j] = (Q_i.K_j + Q_i.posK[idx(i-j)] + K_j.posQ[idx(i-j)]) / scale,  out = softmax_j(s) V
 * qkv_bf16: fused rows (n*T, 3 H 64), q | k | v.  posq / posk: bf16 (2S, H 64) with row stride ld_pos (elements): the layer's
 * query / key projections of the normalised relative embeddings.  idx: int32 [2T - 1], idx[delta + T - 1] in [0, 2S) for
 * delta = i - j, NON-DECREASING WITH STEPS OF AT MOST 1 (the kernel forms only the run of rows a tile can reach; values are
 * clamped to [0, 2S), so a table that breaks this gives wrong numbers, not a stray access).  A pair (i, j) with mask[i] *
 * mask[j] == 0 scores the lowest finite f32: masked keys get probability exactly 0 and a masked query row attends uniformly
 * over all T keys, as HuggingFace's masked_fill + softmax does.  out_bf16 (n*T, H 64).  Scores, bias and probabilities are never
 * written to memory.  1 <= T <= 1024, 1 <= S <= 256, n and H <= 65535; head_dim other than 64 is MMF_E_UNSUPPORTED. */
int mmf_deberta_attn_fwd(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                         const void* mask, int mask_kind, void* out_bf16, int n, int H, int T, int S, int head_dim, float scale,
                         void* stream);
/* The same launch that also writes lse (n, H, T) f32: lse[item][h][i] = m + log(l) of query i's scaled, masked scores (natural
 * log; m the row maximum, l the sum of exp(s - m) over the T keys).  out_bf16 is bit-identical to mmf_deberta_attn_fwd's.  A
 * masked query row's scores are all the lowest finite f32, so its lse is that value again; mmf_deberta_attn_bwd does not use
 * it.  lse 4-byte aligned. */
int mmf_deberta_attn_fwd_lse(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                             const void* mask, int mask_kind, void* out_bf16, float* lse, int n, int H, int T, int S, int head_dim,
                             float scale, void* stream);
/* Backward of the above with respect to q, k, v (the position tables are frozen), c = 1 / scale:
 *   P_ij  = exp(s_ij - lse_i) for a query with mask_i != 0, 1 / T for every key j < T of a masked query (the forward's uniform row)
 *   dS_ij = c P_ij (dO_i.V_j - delta_i) on unmasked pairs, 0 on masked pairs;   delta_i = sum_d dO_i O_i
 *   dV_j  = sum_i P_ij dO_i                                 (masked query rows contribute 1/T dO_i)
 *   dQ_i  = sum_j dS_ij K_j + sum_r A_ir posK[r],   A_ir = sum of dS_ij over {j : idx(i-j) = r}
 *   dK_j  = sum_i dS_ij Q_i + sum_r B_jr posQ[r],   B_jr = sum of dS_ij over {i : idx(i-j) = r}
 * so dQ of a masked query row and dK of a masked key are exactly 0.  out_bf16 / lse: what mmf_deberta_attn_fwd_lse wrote for
 * these operands; dout_bf16 (n*T, H 64) the gradient of out; delta_ws: n*H*T floats of scratch (holds delta afterwards);
 * dqkv_bf16 (n*T, 3 H 64) in qkv's layout: every element of its n*T rows is written (the caller need not zero it), each by one
 * lane in a fixed summation order: no atomics, bitwise repeatable.  Three launches: delta, the dQ pass (one workgroup per 64
 * queries walking the keys), the dK/dV pass (one per 64 keys walking the queries); P and dS are rounded to bf16 as MFMA
 * operands, accumulation is f32, one rounding of the results.  idx: mmf_deberta_attn_fwd's contract, clamped the same way.
 * mmf_deberta_attn_fwd's limits; dout / dqkv 16-byte aligned, lse / delta_ws 4-byte aligned. */
int mmf_deberta_attn_bwd(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                         const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                         float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale, void* stream);
/* mmf_deberta_attn_bwd plus the gradient of the position tables (fine-tuning: the layer's q / k weights also project the relative
 * embeddings), summed over the n items of the call:
 *   dposK[r] += sum_i A_ir Q_i        dposQ[r] += sum_j B_jr K_j        (A_ir / B_jr: the bucket sums of dS above)
 * dqkv_bf16 is bit-identical to mmf_deberta_attn_bwd's for the same operands.  dposq / dposk: f32 (2S, H 64) with row stride ld_dpos
 * (elements); the results are ADDED (the caller zeroes them once, calls accumulate); a row no (i, j) pair of the call maps to
 * has 0 added.  The bucket sums are the bf16 values the position term of dQ / dK reads, contracted over a workgroup's 64 tokens by
 * MFMA into that workgroup's own f32 partial table in `workspace`; a last launch sums the rows the partial tables hold in a fixed
 * order: no floating-point atomics, bitwise repeatable.  workspace: mmf_deberta_attn_bwd_pos_workspace_bytes(n, H, T, S) bytes =
 * 2 n ceil(T / 64) H (2S) 64 floats; it need not be initialised (a row is stored before it is added to or read) and holds
 * nothing afterwards.  Four launches, no memset (a captured graph replays kernel nodes in order).  mmf_deberta_attn_bwd's limits and
 * codes; null dposq / dposk / workspace, ld_dpos < H 64 or a workspace that is too small: MMF_E_SHAPE; dposq / dposk / workspace
 * not 16-byte aligned or ld_dpos not a multiple of 4: MMF_E_ALIGN. */
size_t mmf_deberta_attn_bwd_pos_workspace_bytes(int n, int H, int T, int S);
int mmf_deberta_attn_bwd_pos(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                             const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                             float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale,
                             float* dposq, float* dposk, int ld_dpos, void* workspace, size_t workspace_bytes, void* stream);
/* Training-mode dropout (mmfusion/deberta.py: HuggingFace's DebertaV2Model in train()).  Every mask is a stateless hash of
 * (*rng_state, site, sub-stream, index) by mmf_dropout's counter hash, with p quantised to 2^-32 and c = 1 / (1 - p) as
 * mmf_dropout forms them, and is keyed by the ELEMENT, never by the launch: `item0` is the index, in the whole batch, of the
 * call's first item, so a batch cut into chunks draws what one call would, and a backward regenerates the forward's mask from
 * the same (state, site, item0) instead of reading a stored one.  The codes these four add to the plain entry points': p outside
 * [0, 1) (NaN included), item0 < 0, or a NULL rng_state with a non-zero threshold: MMF_E_SHAPE; rng_state not 8-byte aligned:
 * MMF_E_ALIGN.  Nothing is launched on an error.
 *
 * mmf_deberta_attn_fwd with dropout of the probabilities (softmax -> dropout -> @ V): pair (query i, key j) of head h of item g is
 * kept where the hash of sub-stream (item0 + g) H + h at index i T + j passes, out_i = sum_j keep_ij c P_ij V_j.  The softmax
 * statistics run over the undropped probabilities: lse (NULL: not written) is bit-identical to mmf_deberta_attn_fwd_lse's.  A
 * threshold of 0 (p = 0) runs mmf_deberta_attn_fwd / _lse's own kernels: their bits, and rng_state may be NULL. */
int mmf_deberta_attn_fwd_drop(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                              const void* mask, int mask_kind, void* out_bf16, float* lse, int n, int H, int T, int S, int head_dim,
                              float scale, float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream);
/* mmf_deberta_attn_bwd / mmf_deberta_attn_bwd_pos of that forward (out_bf16 / lse as it wrote them, the same p, state, site and
 * item0): with w_ij = keep_ij c, dS_ij = c' P_ij (w_ij dO_i.V_j - delta_i) (c' = 1 / scale) and dV_j = sum_i w_ij P_ij dO_i; delta,
 * dQ, dK and the table gradients follow from that dS unchanged.  Both passes regenerate the forward's bits.  The plain entry points'
 * operands, launches, limits and codes; dqkv_bf16 of the _pos form is bit-identical to the other's; a threshold of 0 runs the plain
 * kernels. */
int mmf_deberta_attn_bwd_drop(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                              const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                              float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale, float p,
                              const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream);
int mmf_deberta_attn_bwd_pos_drop(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                  const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                                  float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale,
                                  float* dposq, float* dposk, int ld_dpos, void* workspace, size_t workspace_bytes, float p,
                                  const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream);
/* Hidden dropout over `items` items of per_item elements each, one pass (csrc/elementwise.hip; no model's own: Wav2Vec2's hidden
 * sites take it too, mmfusion/wav2vec2.py): element e of item g is kept where the hash of sub-stream item0 + g at index e passes.  bf16 (is_f32 0): out = bf16(fma(y, c, resid)) where kept, resid where dropped: one f32 multiply-add,
 * one rounding; resid_bf16 NULL: 0 (the plain dropout and, on a gradient, its backward).  f32 (is_f32 1, resid_bf16 NULL): out =
 * y c where kept, 0 where dropped.  out may be y or resid.  A threshold of 0 copies (c = 1, everything kept) and still needs
 * rng_state.  per_item % 8 == 0, per_item <= 2^31, items < 2^31 (else MMF_E_UNSUPPORTED); y / resid / out 16-byte aligned. */
int mmf_hidden_dropout(const void* y, const void* resid_bf16, void* out, int is_f32, int64_t items, int64_t per_item, float p,
                       const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream);
/* Backward of mmf_deberta_embed on the embeds route: d_embeds (rows, d) f32 = mask[row] * the LayerNorm input gradient of
 * dout_bf16 (rows, d), the gradient of the kernel's bf16 output.  The row statistics are recomputed in f32 from embeds as the
 * forward computes them; rows with mask 0 are exactly 0.  mmf_deberta_embed's limits on d; embeds / gamma / d_embeds 16-byte
 * aligned, dout 8-byte aligned. */
int mmf_deberta_embed_bwd(const float* embeds, const float* gamma, float eps, const void* mask, int mask_kind, const void* dout_bf16,
                          float* d_embeds, int64_t rows, int d, void* stream);
/* Backward of mmf_deberta_embed on either route with the LayerNorm parameters' gradients (full fine-tuning).  The source row of
 * row r is table[clamp(ids[r])] (ids given; the forward's clamp to [0, vocab)) or embeds[r] (embeds given); exactly one of the two.
 *   d_rows (rows, d) f32  = (accumulate: +=) mask[r] * the LayerNorm input gradient of dout_bf16[r], as mmf_deberta_embed_bwd
 *   dgamma [d] f32       += sum_r dout[r] * mask[r] * xhat[r]          dbeta [d] f32 += sum_r dout[r] * mask[r]
 * On the embeds route without accumulate the d_rows bits are mmf_deberta_embed_bwd's for the same operands.  A row with mask 0
 * is exactly 0 in d_rows (untouched with accumulate), adds nothing to dgamma / dbeta, and its source row is not read.  The column
 * sums go through per-workgroup partial rows in `workspace` (mmf_deberta_embed_bwd_params_workspace_bytes(rows, d) bytes, f32; it
 * need not be initialised and holds nothing afterwards) that a second launch adds in a fixed order: no floating-point atomics,
 * bitwise repeatable.  Two launches.  mmf_deberta_embed's limits on d (else MMF_E_UNSUPPORTED); a null operand, both or neither
 * of ids / embeds, or a workspace that is too small: MMF_E_SHAPE; table / embeds / gamma / d_rows / dgamma / dbeta / workspace not
 * 16-byte aligned, dout or ids not 8-byte aligned: MMF_E_ALIGN.  Nothing is launched on an error. */
size_t mmf_deberta_embed_bwd_params_workspace_bytes(int64_t rows, int d);
int mmf_deberta_embed_bwd_params(const int64_t* ids, const float* embeds, const float* table, int vocab, const float* gamma, float eps,
                                 const void* mask, int mask_kind, const void* dout_bf16, float* d_rows, int accumulate, float* dgamma,
                                 float* dbeta, void* workspace, size_t workspace_bytes, int64_t rows, int d, void* stream);
/* dtable[clamp(ids[r])] += d_rows[r] for the rows r with mask[r] != 0: ids int64 [rows] (mmf_deberta_embed's clamp), d_rows f32
 * (rows, d), dtable f32 (vocab, d); a masked row is not read.  The first unmasked occurrence of a table row owns it: its wave adds
 * the occurrences in ascending row order in registers and reads, adds to and writes the table row once, so every table element is
 * written by one lane once per call, a table row no unmasked id names is not touched, and there are no floating-point atomics:
 * bitwise repeatable.  Nothing is sorted and nothing synchronises with the host (the ids are read on the device only), so a
 * captured graph replays correctly with other ids.  One wave sums all occurrences of an id: a very frequent id is the slow case.
 * d % 4 == 0, d <= 1024, rows <= 2^30 (else MMF_E_UNSUPPORTED); a null operand: MMF_E_SHAPE; d_rows / dtable not 16-byte
 * aligned or ids not 8-byte aligned: MMF_E_ALIGN. */
int mmf_embedding_scatter_add_f32(const int64_t* ids, const void* mask, int mask_kind, const float* d_rows, float* dtable, int64_t rows,
                                  int d, int vocab, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input preparation (mmfusion/prep.py; the reference does this on the host per sample, data/dataset_loaders.py:95-261): what a
 * decoder emits -> what the backbones read.  Every function validates first and launches nothing on an error; an optional
 * per-frame / per-clip device array is NULL for "none".  DESIGN.md section 11 states the geometry, the filter and the RNG keying.
 * ------------------------------------------------------------------------------------------ */
/* frames (N, Hs, Ws, 3) u8 -> pixels (N, 3, H, W) f32.  Output pixel (c, y, x) is the bilinear interpolation (half-pixel centres,
 * no antialiasing, edge replication: sx = (x + 0.5) Ws / W - 0.5 clamped below at 0, x0 = floor(sx), x1 = min(x0 + 1, Ws - 1),
 * the same in y; coordinates in integer arithmetic) of byte (bgr ? 2 - c : c) of the source pixels, then
 * clamp(v / 255 * brightness[n], 0, 1); with flip[n] column x takes the value of column W - 1 - x; a frame with live[n] == 0 is
 * zeros.  live / flip u8 [N], brightness f32 [N].  W % 4 == 0 (else MMF_E_UNSUPPORTED), pixels 16-byte aligned (MMF_E_ALIGN),
 * N <= 65535 and every side <= 16384. */
int mmf_video_prepare(const uint8_t* frames, const uint8_t* live, const float* brightness, const uint8_t* flip, float* pixels,
                      int N, int Hs, int Ws, int H, int W, int bgr, void* stream);
/* The same pixels rounded to bf16 and stored as mmf_vit_patchify stores them: patches (N * (H/P) * (W/P), 3*P*P) bf16, bit-identical
 * to mmf_vit_patchify of mmf_video_prepare's result, which is never written.  mmf_vit_patchify's constraints. */
int mmf_video_prepare_patches(const uint8_t* frames, const uint8_t* live, const float* brightness, const uint8_t* flip,
                              void* patches_bf16, int N, int Hs, int Ws, int H, int W, int P, int bgr, void* stream);
/* wave (B, C, Ls) f32 -> out (B, L) f32 in one launch: mean over the C channels, resampling by new / orig (the rates divided by
 * their gcd), zero padding / truncation to L.  Samples at or past len[b] (int32 [B], NULL: Ls) do not exist; outputs at or past
 * ceil(new len / orig) are 0.  table: f32 (new, 2 width + orig), table[j][k] = g(((k - width) / orig - j / new) base) with
 * base = 0.99 min(orig, new), width = ceil(6 orig / base), g(t) = cos^2(pi t / 12) sinc(pi t) base / orig inside |t| < 6 and 0
 * outside; out[i new + j] = sum_k x[i orig + k - width] table[j][k].  table_elems must be new (2 width + orig) and width the value
 * above (MMF_E_SHAPE).  orig == new takes a NULL table: mono mix and padding only.  B <= 65535, Ls and L below 2^30. */
int mmf_audio_resample(const float* wave, const int* len, const float* table, int64_t table_elems, float* out, int B, int C,
                       int64_t Ls, int64_t L, int orig, int new_, int width, void* stream);
/* x (B, L) f32 -> out (B, L) f32, not in place.  xn[j] = x[j] + 0.01 z(b, j) where noise_on[b] (u8 [B]), z standard normal by
 * Box-Muller from draws 2 j and 2 j + 1 of mmf_dropout's counter hash under the key of (*rng_state, site, b).  With
 * n = stretch_len[b] (int32 [B]; NULL, L or a value below 1: off), out[i] for i < min(n, L) is xn resized L -> n by linear
 * interpolation (half-sample centres, integer coordinates, edge replication) and 0 from there on. */
int mmf_audio_augment(const float* x, float* out, const uint8_t* noise_on, const int* stretch_len, const uint64_t* rng_state,
                      uint32_t site, int B, int64_t L, void* stream);

/* ---- WavLM's gated relative position bias (csrc/wavlm.hip) ----------------------------------------------------------------
 * mmf_wavlm_gate: x (n*T, ldx) bf16, the layer's INPUT rows (H heads of head_dim columns each) -> gate (n, H, T) f32,
 *     gate[b][h][t] = sigmoid(a) (sigmoid(b) head_const[h] - 1) + 2,
 *     a = sum_{o<4} y[o], b = sum_{4<=o<8} y[o], y = lin_w x[b T + t][h head_dim ..] + lin_b
 * with lin_w (8, head_dim) f32 and lin_b (8) f32 shared by all heads (HuggingFace's gru_rel_pos_linear / gru_rel_pos_const).
 * f32 throughout in a fixed summation order: the same bits on every run.  head_dim 64 / 96 (else MMF_E_UNSUPPORTED); a null
 * operand or a non-positive size: MMF_E_SHAPE; x / lin_w not 16-byte aligned, ldx < H head_dim or not a multiple of 8, lin_b /
 * head_const / gate not 4-byte aligned: MMF_E_ALIGN.  Nothing is launched on an error.
 *
 * mmf_attn_fwd_relbias: mmf_attn_fwd_grouped for ONE self-attention problem (Tq == Tk = T, else MMF_E_SHAPE) with
 *     score[b][h][i][j] = scale q_i . k_j + gate[b][h][i] * table[h][j - i + T - 1]
 * gate (B, H, T) f32 as mmf_wavlm_gate writes it, table (H, 2T - 1) f32.  Writes O (bf16) and LSE (f32 (B, H, T), the
 * log-sum-exp of the biased scores).  The (T, T) bias is never formed.  mmf_attn_fwd_grouped's constraints and codes: head_dim
 * 64 / 96 (MMF_E_UNSUPPORTED), null problem / Q / K / V / O / LSE / gate / table (MMF_E_SHAPE), Q / K / V / O 16-byte aligned
 * with row strides >= H head_dim and multiples of 8, LSE / gate / table 4-byte aligned (MMF_E_ALIGN); nothing is launched on
 * an error. */
int mmf_wavlm_gate(const void* x_bf16, int ldx, const float* lin_w, const float* lin_b, const float* head_const, float* gate,
                   int n, int T, int H, int head_dim, void* stream);
int mmf_attn_fwd_relbias(const mmf_attn_problem* problem, int head_dim, float scale, const float* gate, const float* table,
                         void* stream);

/* ---- The BERT family: embedding row, packed key mask, key-masked attention forward (csrc/bert.hip) ---------------------------
 * mmf_bert_embed: out (rows, d) bf16 = LayerNorm((word[ids[r]] | embeds[r]) + type[token_type_ids[r]] + pos[p(r)]), rows =
 * n * T tokens of n items; the rows, gamma and beta are f32, the sum and the LayerNorm are carried in f64 and rounded once.  Exactly one of ids (int64) / embeds (f32 (rows, d)); token_type_ids (int64) may be NULL: row 0.
 * position_rule 0 (BERT): p = t, the token's place in its item.  1 (RoBERTa): on the ids route p = pad + #{ids != pad among the
 * item's tokens 0 .. t} where ids[r] != pad, else pad (HuggingFace's create_position_ids_from_input_ids, counted on the device);
 * on the embeds route p = pad + 1 + t.  Ids, type ids and positions are clamped into their tables (vocab, ntype, npos rows): no
 * input reads outside a table.  d a multiple of 4, at most 1024, rows below 2^31 (MMF_E_UNSUPPORTED); a null operand, both or
 * neither of ids / embeds, rows not a multiple of T, an unknown rule: MMF_E_SHAPE; tables / embeds / gamma / beta / out 16-byte
 * aligned, ids / type ids 8-byte aligned (MMF_E_ALIGN).
 *
 * mmf_mask_pack: an (n, T) mask (mask_kind 0: none, mask NULL; 1: f32; 2: u8; an element is valid when non-zero) -> packed, n rows
 * of mmf_mask_pack_words(T) = 2 + 2 ceil(T / 64) uint32: [0] one past the last valid key (0: none), [1] the count of valid keys,
 * [2 + w] bit k set = key 32 w + k is valid (keys past T: 0).  One launch, nothing on the host.  packed 8-byte aligned.
 *
 * mmf_attn_fwd_keymask: mmf_attn_fwd_grouped for ONE self-attention problem (Tq == Tk = T, else MMF_E_SHAPE) whose keys are
 * masked per item by packed_mask (B rows as mmf_mask_pack writes them): a masked key has probability exactly 0, every query row
 * is computed, an item without a valid key attends uniformly over all T keys (O = the mean of its value rows, LSE = ln T).  Blocks
 * of 32 masked keys are skipped and tiles past an item's last valid key are not read.  Writes O (bf16) and LSE (f32 (B, H, T), over
 * the valid keys).  No atomics: the same bits on every run.  mmf_attn_fwd_relbias's constraints and codes, with packed_mask 8-byte
 * aligned; nothing is launched on an error. */
int mmf_bert_embed(const int64_t* ids, const float* embeds, const int64_t* token_type_ids, const float* word, const float* pos,
                   const float* type, const float* gamma, const float* beta, float eps, int position_rule, int64_t pad,
                   void* out_bf16, int64_t rows, int T, int d, int vocab, int npos, int ntype, void* stream);
int mmf_mask_pack_words(int T);
int mmf_mask_pack(const void* mask, int mask_kind, uint32_t* packed, int n, int T, void* stream);
int mmf_attn_fwd_keymask(const mmf_attn_problem* problem, int head_dim, float scale, const uint32_t* packed_mask, void* stream);

/* ---- Whisper's front end: log-mel features and the padded convolution stem (csrc/whisper.hip) ---------------------------------
 * mmf_whisper_logmel: wave (N, L) f32 at 16 kHz, row stride ld -> HuggingFace WhisperFeatureExtractor's input_features
 * (_np_extract_fbank_features): the clip zero-padded to n_samples, reflect-padded by 200 on both sides, frames of 400 at hop 160
 * times window (f32 [400], the periodic Hann), |DFT|^2 over 201 bins, times mel_fb (201, n_mels) f32, log10(max(., 1e-10)), the
 * last frame dropped (Tm = n_samples / 160 frames), max(x, the clip's own maximum - 8), (x + 4) / 4.  dft is the host's table,
 * f32 (400, 2 MMF_WHISPER_DFT_COLS): dft[k][b] = cos(2 pi b k / 400) and dft[k][MMF_WHISPER_DFT_COLS + b] = sin(2 pi b k / 400) for
 * b < 201, zero columns behind; the product runs on the f32-input MFMA (an f32 fmaf chain in k order) and no sine or cosine is
 * evaluated on the device.  The mel product walks each filter's run of non-zero bins.
 *   features  (N, n_mels, Tm) f32, HuggingFace's layout; may be NULL
 *   window    (N, Tm, Kw) bf16, the first convolution's A operand (kernel 3, padding 1): window[n][t][j n_mels + c] =
 *             bf16(features[n][c][t + j - 1]), zero outside 0 .. Tm - 1 and in columns 3 n_mels .. Kw - 1; may be NULL (not both)
 *   scratch   mmf_whisper_logmel_scratch_bytes(N, n_samples, n_mels) bytes: the raw log spectrum (N, Tm, n_mels) f32 and one maximum
 *             per pass-1 workgroup (the per-clip maximum is the pass boundary)
 * Two launches, no atomics, no host synchronisation: the same bits on every run, graph-capturable.  A null operand, N < 1, L
 * outside 1 .. n_samples, n_samples not a positive multiple of 320, ld < L, Kw < 3 n_mels or not a multiple of 8, a scratch that
 * is too small: MMF_E_SHAPE; n_mels outside {80, 128}, N > 65535: MMF_E_UNSUPPORTED; f32 operands not 4-byte aligned, window /
 * scratch not 16-byte aligned: MMF_E_ALIGN.  Nothing is launched on an error.
 *
 * mmf_whisper_feature_window: features (N, n_mels, Tm) f32 as above -> window, with mmf_whisper_logmel's bits for the same features
 * and its codes.
 *
 * mmf_whisper_gelu_window: x (N, T_in, C) bf16, a raw convolution output, bias f32 [C] -> out (N, T_out, k C) bf16,
 * out[n][t][j C + c] = bf16(gelu(x[n][s t + j - pad][c] + bias[c])) (exact GELU, f32, one rounding), zero where the frame is outside
 * 0 .. T_in - 1; T_out = (T_in + 2 pad - k) / s + 1.  mmf_w2v_gelu_window with a bias and zero padding: the A operand of the next
 * convolution as ONE NT GEMM against its weight repacked to (C_out, k C), column (j, c).  A null operand, a non-positive size,
 * pad < 0, pad >= k, T_in + 2 pad < k: MMF_E_SHAPE; C % 8 != 0, N > 65535, out == x: MMF_E_UNSUPPORTED; x / bias / out not 16-byte
 * aligned: MMF_E_ALIGN.  Nothing is launched on an error.
 *
 * mmf_whisper_stem_out: x (rows, d) bf16, the second convolution's raw output for rows = n T frames, bias f32 [d], pos f32 (T, d) ->
 * out[r][c] = bf16(gelu(x[r][c] + bias[c]) + pos[r % T][c]), the residual stream's first value; out may be x.  A null operand, a
 * non-positive size, rows not a multiple of T: MMF_E_SHAPE; d % 8 != 0: MMF_E_UNSUPPORTED; a pointer not 16-byte aligned:
 * MMF_E_ALIGN.  Nothing is launched on an error. */
#define MMF_WHISPER_DFT_COLS 224
size_t mmf_whisper_logmel_scratch_bytes(int N, int n_samples, int n_mels);
int mmf_whisper_logmel(const float* wave, int64_t ld, const float* window, const float* dft, const float* mel_fb, float* features,
                       void* window_bf16, void* scratch, size_t scratch_bytes, int N, int L, int n_samples, int n_mels, int Kw,
                       void* stream);
int mmf_whisper_feature_window(const float* features, void* window_bf16, int N, int n_mels, int Tm, int Kw, void* stream);
int mmf_whisper_gelu_window(const void* x_bf16, const float* bias, void* out_bf16, int N, int T_in, int C, int k, int s, int pad,
                            void* stream);
int mmf_whisper_stem_out(const void* x_bf16, const float* bias, const float* pos, void* out_bf16, int64_t rows, int T, int d,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMFUSION_H */
