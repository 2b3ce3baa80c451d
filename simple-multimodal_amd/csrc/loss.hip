// The (B, .)-row kernels of the training step's tail and head (round 4): each replaces a chain of stock elementwise launches
// whose work is a few hundred bytes — at these sizes a step pays ~5 us per LAUNCH, so the chains cost 100-200 us each.
//
//   loss_tail_kernel<CE, KD>  the loss tail, value AND the gradient with respect to the logits in one launch; one thread per
//                             sample (C <= 64 logits), B looped.
//     <true, false>           (mmf_fusion_loss) reference training/advanced_trainer.py:139-166: CrossEntropy(label_smoothing)
//                             plus weighted scalar terms (0.1 x the three contrastive losses, 0.5 x distillation) (torch:
//                             log_softmax, nll_loss, smoothing sum, three scalar adds, and the same again backwards: ~35 launches).
//     <false, true>           (mmf_distill_kl) reference models/multimodal_model.py:250-256: T^2 * KL(softmax(t / T) ||
//                             softmax(s / T)), batchmean (torch: the two scaled log_softmax / softmax, kl_div, the T^2 scale and
//                             their backward: 20 launches, counted by tools/distill_bench.py).
//     <true, true>            (mmf_fusion_loss_kd) the CE + sum_j w_j extra_j of <true, false> plus kd_weight * KD as ONE launch,
//                             the gradient with respect to the student logits summed in registers (the distillation step's tail).
//   modality_dropout_kernel   reference models/encoders.py:289-321: per-sample Bernoulli keep masks over the three modalities,
//                             no 1 / (1 - p) rescale, a sample that lost all three gets one back at random; masks drawn from the
//                             build's counter-based hash of (device step state, site, sample) like every other dropout site, the
//                             three (B, d) tensors scaled in the same launch (torch: rand, compare, randint, one_hot, where, any
//                             and three strided copies in front of three row-mask launches).  The same kernel applies a given mask
//                             (backward).
#include "mmf_internal.h"

namespace {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_MAX_EXTRA = 8;

struct LossArgs {
  const float* logits;            // (B, ldl): the CE logits and the KD student
  const float* teacher;           // (B, ldt), KD
  const long long* targets;       // CE
  float* loss;
  float* dlogits;                 // dense (B, C), nullable
  const float* extra[LOSS_MAX_EXTRA];   // CE: device scalars added with weights extra_w
  float extra_w[LOSS_MAX_EXTRA];
  int B, C, ldl, ldt, n_extra;
  float smoothing, T, kd_weight;
};

// ---- cross entropy with label smoothing (reference training/advanced_trainer.py:139-166) ----------------------------------------
// Fast __expf / __logf: the row is max-subtracted, so every exp argument is <= 0 and the sum is >= 1.
struct CeRow { float lse, term; int y; };

__device__ __forceinline__ CeRow ce_row(const float* l, const long long* target, int C, float eps, float invC) {
  CeRow r;
  float mx = -INFINITY;
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, l[c]);
  float se = 0.f, sl = 0.f;
  for (int c = 0; c < C; ++c) { se += __expf(l[c] - mx); sl += l[c]; }
  r.lse = mx + __logf(se);
  r.y = (int)*target;
  const float nll = r.lse - l[r.y];                          // -log p_y
  const float smooth = r.lse - sl * invC;                    // -(1 / C) sum_c log p_c
  r.term = (1.f - eps) * nll + eps * smooth;
  return r;
}

// d(mean_b CE_b) / d l_c of a row from its statistics
__device__ __forceinline__ float ce_grad(const CeRow& r, float l, int c, float eps, float invC, float invB) {
  return (__expf(l - r.lse) - ((c == r.y ? 1.f - eps : 0.f) + eps * invC)) * invB;
}

// ---- knowledge distillation (reference models/multimodal_model.py:222-262) ------------------------------------------------------
// Arithmetic: the KD terms use the ACCURATE expf / logf (OCML, <= 1 ulp each), not __expf / __logf — whose error grows with the
// argument (|x| * 2^-22 relative for the exp of a scaled logit) and which T^2 would then amplify; C <= 64 exps per row cost
// nothing here.  Everything is evaluated from max-subtracted, temperature-scaled logits, z_c = (x_c - max x) / T (one rounded
// difference, one correctly-rounded division, z <= 0), and with Z = sum_c exp(z_c):
//   KL_b = sum_c p_c (zt_c - zs_c) - log(Zt / Zs),   p = softmax(t / T) = exp(zt) / Zt,   q = softmax(s / T) = exp(zs) / Zs
// (sum_c p_c log p_c - sum_c p_c log q_c with the two log-sum-exps folded into one log of a ratio in [1/64, 64]).  A teacher
// probability that underflows to 0 multiplies a finite difference and adds exactly 0 (torch's xlogy); teacher == student gives
// exactly 0.  Error model (worst case; tests/distill_ref.py evaluates exactly this one per test case), u = 2^-24, C <= 64,
// R = the widest (max - min) of a row of s or t, r = R / T: the scaled differences z carry 2u|z|, exp / log 1 ulp, the C-term
// sums C u of their magnitude, the probabilities (C + 4) u relative (the sum Z) plus u |z| absolute (the exponent's argument):
//   |d KL_b| <= u ((4 + 2C) r + 2 r min(r, C) + 2C + 8)
//   |d loss| <= T^2 max_b |d KL_b| + (B / 256 + 10) u |loss|                    (the f32 batch sum: B / 256 terms per thread)
//   |d dstudent[b][c]| <= kd_weight (T / B) (2C + 10) u
// The CE part of <true, true> is the same ce_row / ce_grad as <true, false>, so the combined kernel equals mmf_fusion_loss +
// kd_weight * mmf_distill_kl up to the order of the f32 additions.

// one row's max-subtracted, temperature-scaled statistics; KL(p || q) of the row
struct KdRow { float ms, mt, rZs, rZt, kl; };

__device__ __forceinline__ KdRow kd_row(const float* s, const float* t, int C, float T) {
  KdRow r;
  r.ms = -INFINITY; r.mt = -INFINITY;
  for (int c = 0; c < C; ++c) { r.ms = fmaxf(r.ms, s[c]); r.mt = fmaxf(r.mt, t[c]); }
  float Zs = 0.f, Zt = 0.f;
  for (int c = 0; c < C; ++c) { Zs += expf((s[c] - r.ms) / T); Zt += expf((t[c] - r.mt) / T); }
  r.rZs = 1.f / Zs; r.rZt = 1.f / Zt;
  float kl = 0.f;
  for (int c = 0; c < C; ++c) {
    const float zs = (s[c] - r.ms) / T, zt = (t[c] - r.mt) / T;
    kl += (expf(zt) * r.rZt) * (zt - zs);
  }
  r.kl = kl - logf(Zt / Zs);
  return r;
}

// q_c - p_c of a row from its statistics (recomputed rather than held: a 64-float array indexed by c would live in scratch)
__device__ __forceinline__ float kd_grad(const KdRow& r, float s, float t, float T) {
  return expf((s - r.ms) / T) * r.rZs - expf((t - r.mt) / T) * r.rZt;
}

// loss = [CE] mean_b CE_b + sum_j w_j extra_j  [KD] + kd_weight * T^2 * mean_b KL_b, summed in that order: the KD term first.
template <bool CE, bool KD>
__global__ __launch_bounds__(LOSS_THREADS)
void loss_tail_kernel(const LossArgs a) {
  static_assert(CE || KD, "a loss tail computes CE, KD or both");
  __shared__ float part[CE + KD][LOSS_THREADS / 64];
  const int tid = threadIdx.x;
  const float eps = a.smoothing, invB = 1.f / (float)a.B, invC = 1.f / (float)a.C;
  const float gk = a.kd_weight * a.T * invB;                 // d(kd_weight * T^2 * mean_b KL_b) / ds = kd_weight (T / B) (q - p)
  float acc_ce = 0.f, acc_kl = 0.f;
  for (int b = tid; b < a.B; b += LOSS_THREADS) {            // one sample per thread: C <= 64 logits
    const float* l = a.logits + (size_t)b * a.ldl;
    const float* t = KD ? a.teacher + (size_t)b * a.ldt : nullptr;
    KdRow kr = {};
    CeRow cr = {};
    if (KD) { kr = kd_row(l, t, a.C, a.T); acc_kl += kr.kl; }
    if (CE) { cr = ce_row(l, a.targets + b, a.C, eps, invC); acc_ce += cr.term; }
    if (a.dlogits) {
      float* d = a.dlogits + (size_t)b * a.C;
      for (int c = 0; c < a.C; ++c) {
        float v = KD ? gk * kd_grad(kr, l[c], t[c], a.T) : 0.f;   // the KD term first, the CE term added to it
        if (CE) v = KD ? v + ce_grad(cr, l[c], c, eps, invC, invB) : ce_grad(cr, l[c], c, eps, invC, invB);
        d[c] = v;
      }
    }
  }
  if (CE) acc_ce = wave_sum(acc_ce);
  if (KD) acc_kl = wave_sum(acc_kl);
  if ((tid & 63) == 0) {
    if (CE) part[0][tid >> 6] = acc_ce;
    if (KD) part[CE][tid >> 6] = acc_kl;
  }
  __syncthreads();
  if (tid == 0) {
    float ce = 0.f, kl = 0.f;
    for (int w = 0; w < LOSS_THREADS / 64; ++w) {
      if (CE) ce += part[0][w];
      if (KD) kl += part[CE][w];
    }
    float out = KD ? a.kd_weight * (a.T * a.T) * (kl * invB) : 0.f;
    if (CE) {
      float t = ce * invB;
      for (int j = 0; j < a.n_extra; ++j) t += a.extra_w[j] * a.extra[j][0];
      out = KD ? out + t : t;
    }
    a.loss[0] = out;
  }
}

struct ModDropArgs {
  const float* x[3];
  float* y[3];
  float* keep;                       // [B][3], written (draw) or read (apply)
  const unsigned long long* rng_state;
  unsigned thresh, site;
  int B, d, draw;
};

// one workgroup per sample
__global__ __launch_bounds__(256)
void modality_dropout_kernel(const ModDropArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  float k[3];
  if (a.draw) {
    const unsigned key = mmf_rng_key(*a.rng_state, a.site, 0u);
    bool kp[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) kp[m] = mmf_keep(key, (unsigned)(3 * b + m), a.thresh);
    if (!(kp[0] || kp[1] || kp[2])) kp[mmf_mix32(key ^ (0x51ed270bu + (unsigned)b)) % 3u] = true;   // :308-314: one modality comes back
#pragma unroll
    for (int m = 0; m < 3; ++m) k[m] = kp[m] ? 1.f : 0.f;
    if (tid < 3) a.keep[3 * b + tid] = k[tid];
  } else {
#pragma unroll
    for (int m = 0; m < 3; ++m) k[m] = a.keep[3 * b + m];
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float* x = a.x[m] + (size_t)b * a.d;
    float* y = a.y[m] + (size_t)b * a.d;
    for (int i = 4 * tid; i < a.d; i += 4 * 256) {
      f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + i);
      v *= k[m];
      *reinterpret_cast<f32x4_t*>(y + i) = v;
    }
  }
}

}  // namespace

// The loss tails' argument checks (every refusal is MMF_E_SHAPE) and launch.  Each validator fills the part of the launch
// arguments it has checked; mmf_fusion_loss_kd runs both.
static int loss_ce_args(const char* who, LossArgs& a, const float* logits, int ldl, const int64_t* targets, int B, int C,
                        float label_smoothing, const float* const* extra, const float* extra_w, int n_extra, float* loss) {
  if (!logits || !targets || !loss || B <= 0 || C <= 0 || C > 64 || ldl < C)
    MMF_FAIL(MMF_E_SHAPE, "%s: B=%d C=%d (1..64) ldl=%d", who, B, C, ldl);
  if (n_extra < 0 || n_extra > LOSS_MAX_EXTRA || (n_extra && (!extra || !extra_w)))
    MMF_FAIL(MMF_E_SHAPE, "%s: n_extra=%d out of range [0,%d]", who, n_extra, LOSS_MAX_EXTRA);
  if (!(label_smoothing >= 0.f) || label_smoothing >= 1.f) MMF_FAIL(MMF_E_SHAPE, "%s: label_smoothing must be in [0, 1)", who);
  for (int j = 0; j < n_extra; ++j) {
    if (!extra[j]) MMF_FAIL(MMF_E_SHAPE, "%s: extra[%d] is null", who, j);
    a.extra[j] = extra[j]; a.extra_w[j] = extra_w[j];
  }
  a.logits = logits; a.targets = reinterpret_cast<const long long*>(targets); a.loss = loss;
  a.B = B; a.C = C; a.ldl = ldl; a.n_extra = n_extra; a.smoothing = label_smoothing;
  return MMF_OK;
}

static int loss_kd_args(const char* who, LossArgs& a, const float* student, int lds, const float* teacher, int ldt, int B, int C,
                        float temperature, float* loss) {
  if (!student || !teacher || !loss || B <= 0 || C <= 0 || C > 64 || lds < C || ldt < C)
    MMF_FAIL(MMF_E_SHAPE, "%s: B=%d C=%d (1..64) lds=%d ldt=%d, student / teacher / loss non-null", who, B, C, lds, ldt);
  if (!(__builtin_isfinite(temperature) && temperature > 0.f)) MMF_FAIL(MMF_E_SHAPE, "%s: temperature must be finite and > 0", who);
  a.logits = student; a.teacher = teacher; a.loss = loss;
  a.B = B; a.C = C; a.ldl = lds; a.ldt = ldt; a.T = temperature;
  return MMF_OK;
}

template <bool CE, bool KD>
static int launch_loss_tail(const char* who, LossArgs& a, float* dlogits, void* stream) {
  a.dlogits = dlogits;
  hipLaunchKernelGGL((loss_tail_kernel<CE, KD>), dim3(1), dim3(LOSS_THREADS), 0, static_cast<hipStream_t>(stream), a);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}

extern "C" int mmf_fusion_loss(const float* logits, int ldl, const int64_t* targets, int B, int C, float label_smoothing,
                               const float* const* extra, const float* extra_w, int n_extra, float* loss, float* dlogits,
                               void* stream) {
  LossArgs a = {};
  if (int rc = loss_ce_args("mmf_fusion_loss", a, logits, ldl, targets, B, C, label_smoothing, extra, extra_w, n_extra, loss))
    return rc;
  return launch_loss_tail<true, false>("mmf_fusion_loss", a, dlogits, stream);
}

extern "C" int mmf_modality_dropout(const float* const* x, float* const* y, float* keep, int B, int d, float p,
                                    const uint64_t* rng_state, uint32_t site, int draw, void* stream) {
  if (!x || !y || !keep || B <= 0 || d <= 0 || (d & 3)) MMF_FAIL(MMF_E_SHAPE, "mmf_modality_dropout: B=%d d=%d (d %% 4 == 0)", B, d);
  if (draw && (!rng_state || !(p >= 0.f) || p >= 1.f)) MMF_FAIL(MMF_E_SHAPE, "mmf_modality_dropout: drawing needs rng_state and 0 <= p < 1");
  ModDropArgs a = {};
  for (int m = 0; m < 3; ++m) {
    if (!x[m] || !y[m] || !mmf_aligned16(x[m]) || !mmf_aligned16(y[m])) MMF_FAIL(MMF_E_ALIGN, "mmf_modality_dropout: null or misaligned operand %d", m);
    a.x[m] = x[m]; a.y[m] = y[m];
  }
  a.keep = keep; a.rng_state = reinterpret_cast<const unsigned long long*>(rng_state);
  a.thresh = draw ? mmf_drop_thresh(p) : 0u; a.site = site; a.B = B; a.d = d; a.draw = draw;
  hipLaunchKernelGGL(modality_dropout_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  MMF_CHECK_LAUNCH("mmf_modality_dropout");
  return MMF_OK;
}

extern "C" int mmf_distill_kl(const float* student, int lds, const float* teacher, int ldt, int B, int C, float temperature,
                              float* loss, float* dstudent, void* stream) {
  LossArgs a = {};
  if (int rc = loss_kd_args("mmf_distill_kl", a, student, lds, teacher, ldt, B, C, temperature, loss)) return rc;
  a.kd_weight = 1.f;
  return launch_loss_tail<false, true>("mmf_distill_kl", a, dstudent, stream);
}

extern "C" int mmf_fusion_loss_kd(const float* logits, int ldl, const int64_t* targets, int B, int C, float label_smoothing,
                                  const float* const* extra, const float* extra_w, int n_extra,
                                  const float* teacher, int ldt, float temperature, float kd_weight,
                                  float* loss, float* dlogits, void* stream) {
  const char* who = "mmf_fusion_loss_kd";
  LossArgs a = {};
  if (int rc = loss_ce_args(who, a, logits, ldl, targets, B, C, label_smoothing, extra, extra_w, n_extra, loss)) return rc;
  if (int rc = loss_kd_args(who, a, logits, ldl, teacher, ldt, B, C, temperature, loss)) return rc;
  if (!__builtin_isfinite(kd_weight)) MMF_FAIL(MMF_E_SHAPE, "%s: kd_weight must be finite", who);
  a.kd_weight = kd_weight;
  return launch_loss_tail<true, true>(who, a, dlogits, stream);
}
