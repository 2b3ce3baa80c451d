// Grouped fused attention for the fusion path (q*scale, QK^T, softmax, P.V of F.multi_head_attention_forward as called at
// models/fusion_layers.py:161-163,204): C-ABI entry points and operand validation.  The kernels are in attention2.hip
// (forward with log-sum-exp; recompute backward: dQ kernel + dK/dV kernel, no atomics, deterministic).  All attentions of
// a MulT stage (6 cross or 3 self, unequal Tq/Tk) go out as ONE launch.  Rounds 1-2 kept superseded kernel generations here
// and in attention3.hip / attention4.hip behind mmf_attn_select_impl; round 3 removed them (git history has them,
// DESIGN.md section 5 their measurements).
#include "attn_helpers.h"
#include <stdlib.h>

namespace {

int validate(const char* who, const mmf_attn_problem* p, int n, int head_dim, bool bwd) {
  if (!p || n <= 0 || n > MMF_ATTN_MAX_PROBLEMS) MMF_FAIL(MMF_E_SHAPE, "%s: num_problems=%d out of range", who, n);
  if (head_dim != 64 && head_dim != 96) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: head_dim=%d (supported: 64, 96)", who, head_dim);
  for (int i = 0; i < n; ++i) {
    const mmf_attn_problem& q = p[i];
    if (q.B <= 0 || q.H <= 0 || q.Tq <= 0 || q.Tk <= 0) MMF_FAIL(MMF_E_SHAPE, "%s[%d]: B=%d H=%d Tq=%d Tk=%d", who, i, q.B, q.H, q.Tq, q.Tk);
    const int w = q.H * head_dim;
    if (q.ldq < w || q.ldk < w || q.ldv < w || q.ldo < w || (q.ldq & 7) || (q.ldk & 7) || (q.ldv & 7) || (q.ldo & 7))
      MMF_FAIL(MMF_E_ALIGN, "%s[%d]: row strides must be >= H*head_dim and multiples of 8", who, i);
    if (!q.Q || !q.K || !q.V || !q.O || !q.LSE) MMF_FAIL(MMF_E_SHAPE, "%s[%d]: null operand", who, i);
    if (!mmf_aligned16(q.Q) || !mmf_aligned16(q.K) || !mmf_aligned16(q.V) || !mmf_aligned16(q.O))
      MMF_FAIL(MMF_E_ALIGN, "%s[%d]: Q/K/V/O must be 16-byte aligned", who, i);
    if (bwd) {
      if (!q.dO || !q.delta || !q.dQ || !q.dK || !q.dV) MMF_FAIL(MMF_E_SHAPE, "%s[%d]: null gradient operand", who, i);
      if (!mmf_aligned16(q.dO) || !mmf_aligned16(q.dQ) || !mmf_aligned16(q.dK) || !mmf_aligned16(q.dV))
        MMF_FAIL(MMF_E_ALIGN, "%s[%d]: gradient pointers must be 16-byte aligned", who, i);
    }
  }
  return MMF_OK;
}

// the probability rule of every entry with dropout
int validate_prob(const char* who, float dropout_p, const uint64_t* rng_state) {
  if (!(dropout_p >= 0.f) || dropout_p >= 1.f || (dropout_p > 0.f && !rng_state))
    MMF_FAIL(MMF_E_SHAPE, "%s: dropout needs 0 <= p < 1 and an rng_state", who);
  return MMF_OK;
}

// the dropout stream id is problem * 4096 + b*H + h: past 4096 (b, h) pairs a problem would draw its successor's masks
int validate_dropout(const char* who, const mmf_attn_problem* p, int n, float dropout_p, const uint64_t* rng_state) {
  if (int rc = validate_prob(who, dropout_p, rng_state)) return rc;
  for (int i = 0; dropout_p > 0.f && i < n; ++i)
    if ((long long)p[i].B * p[i].H > 4096)
      MMF_FAIL(MMF_E_SHAPE, "%s[%d]: dropout needs B*H <= 4096 (B=%d H=%d)", who, i, p[i].B, p[i].H);
  return MMF_OK;
}

}  // namespace

int mmf_attn_fwd2_launch(const mmf_attn_problem* problems, int n, int head_dim, float scale, float drop_p,
                         const uint64_t* rng_state, uint32_t site, hipStream_t s, uint32_t stream_base = 0u);
int mmf_attn_bwd2_launch(const mmf_attn_problem* problems, int n, int head_dim, float scale, float drop_p,
                         const uint64_t* rng_state, uint32_t site, hipStream_t s, bool given_delta = false, uint32_t stream_base = 0u);

namespace {

// The _keyed entries: the dropout stream id is problem * 4096 + stream_base + b*H + h.  One problem may take any base (its ids must
// not wrap); several keep every id of a problem below its successor's first
int validate_keyed(const char* who, const mmf_attn_problem* p, int n, float dropout_p, const uint64_t* rng_state, uint32_t stream_base) {
  if (int rc = validate_prob(who, dropout_p, rng_state)) return rc;
  if (reinterpret_cast<uintptr_t>(rng_state) & 7u) MMF_FAIL(MMF_E_ALIGN, "%s: rng_state must be 8-byte aligned", who);
  for (int i = 0; dropout_p > 0.f && i < n; ++i) {
    const long long last = (long long)stream_base + (long long)p[i].B * p[i].H;
    if (n > 1 ? last > 4096 : last > 0xffffffffLL)
      MMF_FAIL(MMF_E_SHAPE, "%s[%d]: stream_base=%u + B*H=%lld leaves the problem's stream ids (4096 per problem of a group, 2^32 alone)",
               who, i, stream_base, (long long)p[i].B * p[i].H);
  }
  return MMF_OK;
}

// what mmf_attn_bwd_grouped_uniform and _pooled check alike: the operands, then the workspace
int validate_uniform(const char* fn, const mmf_attn_problem* problems, int num_problems, int head_dim, const void* workspace, size_t workspace_bytes) {
  if (int rc = validate(fn, problems, num_problems, head_dim, true)) return rc;
  const size_t need = mmf_attn_bwd_grouped_uniform_workspace_bytes(problems, num_problems);
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3u) || workspace_bytes < need)
    MMF_FAIL(MMF_E_SHAPE, "%s: workspace of %zu bytes (4-byte aligned) required", fn, need);
  return MMF_OK;
}

// delta[b][h][i] = sum_j p_ij dp_ij in f32, p_ij = exp(scale q_i . k_j - LSE_i) and dp_ij = dO_i . v_j from the bf16 operands: the
// softmax backward's row term as the definition has it.  (The backward kernels' own delta = dO . O reads the bf16 O, so a row of
// dS sums to dO . (O - bf16(O)) instead of zero: an absolute residue that gradients much smaller than |dO| |O| do not cover.)
// One thread per query row with q and dO in registers; the keys and values of 32 rows at a time in LDS, read as broadcasts.
// Drop = one MmfItemDrop, item0 carrying the stream base (the dropout form: delta_i = sum_j p_ij w_ij dp_ij with w = keep c drawn as the forward drew it, stream
// item0 + b*H + h, index i Tk + j; p from the undropped LSE) or nothing: the plain instantiation keeps its argument block.
constexpr int DELTA_THREADS = 256, DELTA_KEYS = 32;
template <int DH, typename... Drop>
__global__ __launch_bounds__(DELTA_THREADS)
void attn_delta_kernel(const mmf_attn_problem P, float scale, const Drop... dr) {
  constexpr bool DROP = sizeof...(Drop) != 0;
  __shared__ __attribute__((aligned(16))) unsigned short sk[DELTA_KEYS * DH], sv[DELTA_KEYS * DH];
  const int h = blockIdx.y, b = blockIdx.z, i = blockIdx.x * DELTA_THREADS + threadIdx.x;
  const int Tq = P.Tq, Tk = P.Tk;
  const bool live = i < Tq;
  const unsigned short* Q = static_cast<const unsigned short*>(P.Q) + ((size_t)b * Tq + (live ? i : 0)) * P.ldq + h * DH;
  const unsigned short* dO = static_cast<const unsigned short*>(P.dO) + ((size_t)b * Tq + (live ? i : 0)) * P.ldo + h * DH;
  const unsigned short* K = static_cast<const unsigned short*>(P.K) + (size_t)b * Tk * P.ldk + h * DH;
  const unsigned short* V = static_cast<const unsigned short*>(P.V) + (size_t)b * Tk * P.ldv + h * DH;
  float q[DH], g[DH];
#pragma unroll
  for (int c = 0; c < DH / 8; ++c) {
    float t[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(Q + c * 8), t);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[c * 8 + e] = t[e] * scale;
    unpack8(*reinterpret_cast<const u32x4_t*>(dO + c * 8), t);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[c * 8 + e] = t[e];
  }
  const size_t at = ((size_t)b * P.H + h) * Tq + (live ? i : 0);
  const float lse = P.LSE[at];
  float acc = 0.f;
  unsigned dkey = 0u, dthresh = 0u;
  float dinv = 1.f;
  if constexpr (DROP) {
    const MmfItemDrop d = (dr, ...);
    dkey = mmf_rng_key(*d.state, d.site, d.item0 + (unsigned)(b * P.H + h));
    dthresh = d.thresh;
    dinv = d.inv_keep;
  }
  const unsigned qidx = (unsigned)i * (unsigned)Tk;
  for (int j0 = 0; j0 < Tk; j0 += DELTA_KEYS) {
    __syncthreads();
    for (int v = threadIdx.x; v < DELTA_KEYS * DH / 8; v += DELTA_THREADS) {
      const int r = v / (DH / 8), c = v - r * (DH / 8);
      u32x4_t kk = {0u, 0u, 0u, 0u}, vv = kk;
      if (j0 + r < Tk) {
        kk = *reinterpret_cast<const u32x4_t*>(K + (size_t)(j0 + r) * P.ldk + c * 8);
        vv = *reinterpret_cast<const u32x4_t*>(V + (size_t)(j0 + r) * P.ldv + c * 8);
      }
      *reinterpret_cast<u32x4_t*>(sk + v * 8) = kk;
      *reinterpret_cast<u32x4_t*>(sv + v * 8) = vv;
    }
    __syncthreads();
    const int nk = Tk - j0 < DELTA_KEYS ? Tk - j0 : DELTA_KEYS;
    for (int r = 0; r < nk; ++r) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < DH / 8; ++c) {
        float t[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(sk + r * DH + c * 8), t);
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(q[c * 8 + e], t[e], s);
        unpack8(*reinterpret_cast<const u32x4_t*>(sv + r * DH + c * 8), t);
#pragma unroll
        for (int e = 0; e < 8; ++e) dp = fmaf(g[c * 8 + e], t[e], dp);
      }
      if constexpr (DROP) dp = mmf_keep(dkey, qidx + (unsigned)(j0 + r), dthresh) ? dp * dinv : 0.f;       // dp through the forward's mask
      acc = fmaf(expf(s - lse), dp, acc);
    }
  }
  if (live) P.delta[at] = acc;
}

}  // namespace

// Tuning hook kept for ABI stability: one kernel generation is left, so only 0 (automatic) and 2 are accepted.
extern "C" int mmf_attn_select_impl(int impl) {
  if (impl != 0 && impl != 2)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_attn_select_impl: impl=%d (only generation 2 is built: 0 or 2)", impl);
  return MMF_OK;
}

extern "C" int mmf_attn_fwd_grouped_ex(const mmf_attn_problem* problems, int num_problems, int head_dim,
                                       float scale, float dropout_p, const uint64_t* rng_state, uint32_t site,
                                       void* stream) {
  if (int rc = validate("mmf_attn_fwd_grouped", problems, num_problems, head_dim, false)) return rc;
  if (int rc = validate_dropout("mmf_attn_fwd_grouped_ex", problems, num_problems, dropout_p, rng_state)) return rc;
  return mmf_attn_fwd2_launch(problems, num_problems, head_dim, scale, dropout_p, rng_state, site,
                              static_cast<hipStream_t>(stream));
}

extern "C" int mmf_attn_bwd_grouped_ex(const mmf_attn_problem* problems, int num_problems, int head_dim,
                                       float scale, float dropout_p, const uint64_t* rng_state, uint32_t site,
                                       void* stream) {
  if (int rc = validate("mmf_attn_bwd_grouped", problems, num_problems, head_dim, true)) return rc;
  if (int rc = validate_dropout("mmf_attn_bwd_grouped_ex", problems, num_problems, dropout_p, rng_state)) return rc;
  return mmf_attn_bwd2_launch(problems, num_problems, head_dim, scale, dropout_p, rng_state, site,
                              static_cast<hipStream_t>(stream));
}

extern "C" int mmf_attn_fwd_grouped(const mmf_attn_problem* problems, int num_problems, int head_dim,
                                    float scale, void* stream) {
  return mmf_attn_fwd_grouped_ex(problems, num_problems, head_dim, scale, 0.f, nullptr, 0u, stream);
}

extern "C" int mmf_attn_bwd_grouped(const mmf_attn_problem* problems, int num_problems, int head_dim,
                                    float scale, void* stream) {
  return mmf_attn_bwd_grouped_ex(problems, num_problems, head_dim, scale, 0.f, nullptr, 0u, stream);
}

// mmf_attn_bwd_grouped with delta as an INPUT (f32 [B*H*Tq] per problem, e.g. mmf_attn_delta_f32's): the dQ kernel reads it
// instead of forming dO . O, the dK/dV kernel reads it as it always does.  The dropout form is mmf_attn_bwd_grouped_delta_keyed.
extern "C" int mmf_attn_bwd_grouped_delta(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, void* stream) {
  if (int rc = validate("mmf_attn_bwd_grouped_delta", problems, num_problems, head_dim, true)) return rc;
  return mmf_attn_bwd2_launch(problems, num_problems, head_dim, scale, 0.f, nullptr, 0u, static_cast<hipStream_t>(stream), true);
}

// ---- the uniform backward: one output-gradient row per batch row (include/mmfusion.h; kernels in attention2.hip) ---------------
int mmf_attn_bwd2u_launch(const mmf_attn_problem* problems, int n, int head_dim, float scale, float* cws, hipStream_t s,
                          const void* const* dys = nullptr, int lddy = 0);

extern "C" int mmf_attn_bwd_grouped_uniform_available(int head_dim, float dropout_p) {
  return (head_dim == 64 || head_dim == 96) && dropout_p == 0.f;
}

extern "C" size_t mmf_attn_bwd_grouped_uniform_workspace_bytes(const mmf_attn_problem* problems, int num_problems) {
  size_t n = 0;
  for (int i = 0; problems && i < num_problems; ++i)
    if (problems[i].B > 0 && problems[i].H > 0 && problems[i].Tk > 0) n += (size_t)problems[i].B * problems[i].H * problems[i].Tk;
  return n * sizeof(float);
}

extern "C" int mmf_attn_bwd_grouped_uniform(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = validate_uniform("mmf_attn_bwd_grouped_uniform", problems, num_problems, head_dim, workspace, workspace_bytes)) return rc;
  return mmf_attn_bwd2u_launch(problems, num_problems, head_dim, scale, static_cast<float*>(workspace), static_cast<hipStream_t>(stream));
}

// ... with dO made on the way: dys[i] is problem i's (B, lddy) bf16 gradient of the POOLED output (the mean over Tq); the call writes
// dO[b][:] = bf16(dys[i][b][:] / Tq) into the problem's (B, ldo) dO buffer — what mmf_meanpool_cat_bwd writes Tq times — and goes on
// as mmf_attn_bwd_grouped_uniform.
extern "C" int mmf_attn_bwd_grouped_pooled(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale,
                                           const void* const* dys, int lddy, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "mmf_attn_bwd_grouped_pooled";
  if (int rc = validate_uniform(fn, problems, num_problems, head_dim, workspace, workspace_bytes)) return rc;
  if (!dys || (lddy & 7)) MMF_FAIL(MMF_E_ALIGN, "%s: lddy=%d (a multiple of 8) and the gradient pointers are required", fn, lddy);
  for (int i = 0; i < num_problems; ++i) {
    if (!dys[i] || !mmf_aligned16(dys[i]) || lddy < problems[i].H * head_dim)
      MMF_FAIL(MMF_E_ALIGN, "%s[%d]: the pooled gradient must be 16-byte aligned with lddy >= H*head_dim", fn, i);
  }
  return mmf_attn_bwd2u_launch(problems, num_problems, head_dim, scale, static_cast<float*>(workspace), static_cast<hipStream_t>(stream), dys, lddy);
}

namespace {
int delta_launch(const char* fn, const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, const MmfItemDrop* dr, void* stream) {
  if (int rc = validate(fn, problems, num_problems, head_dim, false)) return rc;
  for (int i = 0; i < num_problems; ++i) {
    if (!problems[i].dO || !problems[i].delta) MMF_FAIL(MMF_E_SHAPE, "%s[%d]: null gradient operand", fn, i);
    if (!mmf_aligned16(problems[i].dO)) MMF_FAIL(MMF_E_ALIGN, "%s[%d]: gradient pointers must be 16-byte aligned", fn, i);
    if (problems[i].H > 65535 || problems[i].B > 65535) MMF_FAIL(MMF_E_UNSUPPORTED, "%s[%d]: B and H at most 65535", fn, i);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < num_problems; ++i) {
    const mmf_attn_problem& p = problems[i];
    const dim3 grid((p.Tq + DELTA_THREADS - 1) / DELTA_THREADS, p.H, p.B);
    if (dr) {
      MmfItemDrop d = *dr;
      d.item0 += (unsigned)i * 4096u;
      attn_select(head_dim, true, [&](auto dh, auto) { hipLaunchKernelGGL((attn_delta_kernel<dh(), MmfItemDrop>), grid, dim3(DELTA_THREADS), 0, s, p, scale, d); });
    } else {
      attn_select(head_dim, false, [&](auto dh, auto) { hipLaunchKernelGGL(attn_delta_kernel<dh()>, grid, dim3(DELTA_THREADS), 0, s, p, scale); });
    }
    MMF_CHECK_LAUNCH(fn);
  }
  return MMF_OK;
}
}  // namespace

extern "C" int mmf_attn_delta_f32(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, void* stream) {
  return delta_launch("mmf_attn_delta_f32", problems, num_problems, head_dim, scale, nullptr, stream);
}

// ---- the _keyed entries: dropout of the probabilities with a caller-chosen base of the stream id (include/mmfusion.h) ----------
extern "C" int mmf_attn_fwd_grouped_keyed(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, float dropout_p,
                                          const uint64_t* rng_state, uint32_t site, uint32_t stream_base, void* stream) {
  const char* fn = "mmf_attn_fwd_grouped_keyed";
  if (int rc = validate(fn, problems, num_problems, head_dim, false)) return rc;
  if (int rc = validate_keyed(fn, problems, num_problems, dropout_p, rng_state, stream_base)) return rc;
  return mmf_attn_fwd2_launch(problems, num_problems, head_dim, scale, dropout_p, rng_state, site, static_cast<hipStream_t>(stream), stream_base);
}

extern "C" int mmf_attn_delta_f32_keyed(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, float dropout_p,
                                        const uint64_t* rng_state, uint32_t site, uint32_t stream_base, void* stream) {
  const char* fn = "mmf_attn_delta_f32_keyed";
  if (int rc = validate(fn, problems, num_problems, head_dim, false)) return rc;
  if (int rc = validate_keyed(fn, problems, num_problems, dropout_p, rng_state, stream_base)) return rc;
  const unsigned thresh = (dropout_p > 0.f && rng_state) ? mmf_drop_thresh(dropout_p) : 0u;
  if (thresh == 0u) return delta_launch(fn, problems, num_problems, head_dim, scale, nullptr, stream);
  const MmfItemDrop d = {reinterpret_cast<const unsigned long long*>(rng_state), site, thresh, stream_base, mmf_inv_keep(thresh)};
  return delta_launch(fn, problems, num_problems, head_dim, scale, &d, stream);
}

extern "C" int mmf_attn_bwd_grouped_delta_keyed(const mmf_attn_problem* problems, int num_problems, int head_dim, float scale, float dropout_p,
                                                const uint64_t* rng_state, uint32_t site, uint32_t stream_base, void* stream) {
  const char* fn = "mmf_attn_bwd_grouped_delta_keyed";
  if (int rc = validate(fn, problems, num_problems, head_dim, true)) return rc;
  if (int rc = validate_keyed(fn, problems, num_problems, dropout_p, rng_state, stream_base)) return rc;
  return mmf_attn_bwd2_launch(problems, num_problems, head_dim, scale, dropout_p, rng_state, site, static_cast<hipStream_t>(stream), true, stream_base);
}
