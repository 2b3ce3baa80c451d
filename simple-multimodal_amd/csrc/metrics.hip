// Evaluation metrics of one batch as one launch (mmf_eval_accumulate).  Replaces the per-batch tail of the reference's
// evaluation loops — training/advanced_trainer.py:209-263 (validate), :607-660 (evaluate_robustness) and
// evaluate_model.py:55-203 (evaluate_dataset) — where torch runs CrossEntropyLoss(label_smoothing), softmax and argmax per
// head and the host then syncs on .item() and three .cpu() copies.  Here everything the metrics need is added to
// device-resident accumulators, and the host reads them once at the end of the pass.
//
//   eval_accumulate_kernel   ONE workgroup of 4 waves.  One wave per row, lane = class (C <= 64 fits one wave64), every
//                            row reduction a __shfl_xor butterfly (all lanes end with the same bits).  Per head: the
//                            (target, prediction) counts of the batch go to a C x C int32 tile in LDS, which is then added
//                            to the int64 confusion accumulator, one cell per thread; per wave the main head's float sums
//                            run in f64 in row order and are combined in wave order.  No global atomics and no protocol
//                            between workgroups: one read-modify-write of the accumulators per launch, ordered with the
//                            next launch by the stream.  The result is the same bits on every run.
#include "mmf_internal.h"

namespace {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_WAVES = EVAL_THREADS / MMF_WAVE;
constexpr int EVAL_MAX_C = 64;
constexpr int EVAL_NSUMS = MMF_EVAL_NSUMS;   // loss sum, sum max-prob, sum max-prob^2, sum max-prob of correct rows

struct EvalArgs {
  const float* logits[MMF_EVAL_MAX_HEADS];
  int ld[MMF_EVAL_MAX_HEADS];
  const long long* targets;
  long long* counts;                   // [heads][C][C] confusion, then invalid, then batches
  double* sums;                        // [EVAL_NSUMS]
  long long* pred_out;                 // (capacity,), nullable
  long long* target_out;               // (capacity,), nullable
  float* prob_out;                     // (capacity, C), nullable
  long long row0;
  int heads, B, C;
  float smoothing;
};

// torch.argmax's order: a NaN beats any number and the first NaN wins; otherwise the larger value, and among equal values
// the lower index.  A strict total order, so the butterfly leaves every lane with the same (value, index).
__device__ __forceinline__ bool eval_better(float va, int ia, float vb, int ib) {
  const bool na = __builtin_isnan(va), nb = __builtin_isnan(vb);
  if (na != nb) return na;
  if (na || va == vb) return ia < ib;
  return va > vb;
}

__global__ __launch_bounds__(EVAL_THREADS)
void eval_accumulate_kernel(const EvalArgs a) {
  __shared__ int tile[EVAL_MAX_C * EVAL_MAX_C];
  __shared__ double part[EVAL_WAVES][EVAL_NSUMS];
  __shared__ int part_invalid[EVAL_WAVES];
  const int tid = threadIdx.x, lane = tid & (MMF_WAVE - 1), wave = tid / MMF_WAVE;
  const int C = a.C, CC = C * C;
  const bool live = lane < C;
  const float eps = a.smoothing, invC = 1.f / (float)C;
  double acc[EVAL_NSUMS] = {0.0, 0.0, 0.0, 0.0};
  int invalid = 0;

  for (int h = 0; h < a.heads; ++h) {
    for (int i = tid; i < CC; i += EVAL_THREADS) tile[i] = 0;
    __syncthreads();
    const float* L = a.logits[h];
    for (int r = wave; r < a.B; r += EVAL_WAVES) {
      const float v = live ? L[(size_t)r * a.ld[h] + lane] : -INFINITY;
      float bv = v;
      int bi = lane;                                           // lanes >= C: -inf at an index above every class
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, MMF_WAVE);
        const int oi = __shfl_xor(bi, o, MMF_WAVE);
        if (eval_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      const long long y64 = a.targets[r];
      const bool valid = y64 >= 0 && y64 < (long long)C;
      const int y = valid ? (int)y64 : 0;                      // never an index unless valid
      if (lane == 0 && valid) atomicAdd(&tile[y * C + bi], 1);
      if (h != 0) continue;

      // main head: softmax with the row max bv subtracted (accurate expf / logf), the CE of torch's label smoothing
      const float e = live ? expf(v - bv) : 0.f;
      const float s = wave_sum(e);
      const float sl = wave_sum(live ? v : 0.f);
      const float ly = __shfl(v, y, MMF_WAVE);
      const float ls = logf(s);
      const float nll = (bv - ly) + ls;                        // -log p_y
      const float smooth = (bv + ls) - sl * invC;              // -(1 / C) sum_c log p_c
      const float maxp = 1.f / s;                              // p at the argmax: exp(0) / s
      const long long row = a.row0 + r;
      if (a.prob_out && live) a.prob_out[row * C + lane] = e / s;
      if (lane == 0) {
        if (a.pred_out) a.pred_out[row] = bi;
        if (a.target_out) a.target_out[row] = y64;
      }
      if (valid) {
        acc[0] += (double)((1.f - eps) * nll + eps * smooth);
        if (bi == y) acc[3] += (double)maxp;
      } else {
        ++invalid;
      }
      acc[1] += (double)maxp;
      acc[2] += (double)maxp * (double)maxp;
    }
    __syncthreads();
    long long* conf = a.counts + (size_t)h * CC;
    for (int i = tid; i < CC; i += EVAL_THREADS)
      if (tile[i]) conf[i] += tile[i];
    __syncthreads();                                           // the tile is zeroed again for the next head
  }

  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < EVAL_NSUMS; ++k) part[wave][k] = acc[k];
    part_invalid[wave] = invalid;
  }
  __syncthreads();
  if (tid == 0) {
    double t[EVAL_NSUMS] = {0.0, 0.0, 0.0, 0.0};
    long long inv = 0;
    for (int w = 0; w < EVAL_WAVES; ++w) {
#pragma unroll
      for (int k = 0; k < EVAL_NSUMS; ++k) t[k] += part[w][k];
      inv += part_invalid[w];
    }
    a.sums[0] += t[0] / (double)a.B;                           // the batch's mean loss (rows with invalid targets add 0)
#pragma unroll
    for (int k = 1; k < EVAL_NSUMS; ++k) a.sums[k] += t[k];
    long long* tail = a.counts + (size_t)a.heads * CC;
    tail[0] += inv;
    tail[1] += 1;
  }
}

}  // namespace

static bool eval_aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

extern "C" int mmf_eval_accumulate(const float* const* logits, const int* ld, int n_heads, const int64_t* targets, int B,
                                   int C, float label_smoothing, int64_t* counts, double* sums, int64_t* pred_out,
                                   int64_t* target_out, float* prob_out, int64_t row0, int64_t capacity, void* stream) {
  const char* who = "mmf_eval_accumulate";
  if (!logits || !ld || n_heads < 1 || n_heads > MMF_EVAL_MAX_HEADS)
    MMF_FAIL(MMF_E_SHAPE, "%s: n_heads=%d (1..%d), logits / ld non-null", who, n_heads, MMF_EVAL_MAX_HEADS);
  if (B <= 0 || C < 1 || C > EVAL_MAX_C) MMF_FAIL(MMF_E_SHAPE, "%s: B=%d C=%d (1..%d)", who, B, C, EVAL_MAX_C);
  if (!targets || !counts || !sums) MMF_FAIL(MMF_E_SHAPE, "%s: targets / counts / sums must be non-null", who);
  if (!(label_smoothing >= 0.f) || label_smoothing >= 1.f) MMF_FAIL(MMF_E_SHAPE, "%s: label_smoothing must be in [0, 1)", who);
  const bool collect = pred_out || target_out || prob_out;
  if (collect && (row0 < 0 || capacity < 0 || row0 > capacity - B))
    MMF_FAIL(MMF_E_SHAPE, "%s: rows [%lld, %lld) outside the output capacity %lld", who, (long long)row0,
             (long long)row0 + B, (long long)capacity);
  EvalArgs a = {};
  for (int h = 0; h < n_heads; ++h) {
    if (!logits[h] || ld[h] < C) MMF_FAIL(MMF_E_SHAPE, "%s: head %d: null logits or row stride %d < C=%d", who, h, ld[h], C);
    if (!eval_aligned(logits[h], 4)) MMF_FAIL(MMF_E_ALIGN, "%s: head %d: logits not 4-byte aligned", who, h);
    a.logits[h] = logits[h]; a.ld[h] = ld[h];
  }
  if (!eval_aligned(targets, 8) || !eval_aligned(counts, 8) || !eval_aligned(sums, 8) || !eval_aligned(pred_out, 8) ||
      !eval_aligned(target_out, 8) || !eval_aligned(prob_out, 4))
    MMF_FAIL(MMF_E_ALIGN, "%s: misaligned targets / accumulators / outputs", who);
  a.targets = reinterpret_cast<const long long*>(targets);
  a.counts = reinterpret_cast<long long*>(counts);
  a.sums = sums;
  a.pred_out = reinterpret_cast<long long*>(pred_out);
  a.target_out = reinterpret_cast<long long*>(target_out);
  a.prob_out = prob_out;
  a.row0 = row0; a.heads = n_heads; a.B = B; a.C = C; a.smoothing = label_smoothing;
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(EVAL_THREADS), 0, static_cast<hipStream_t>(stream), a);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}
