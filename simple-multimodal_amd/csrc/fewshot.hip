// Episode head of FewShotModel (reference models/multimodal_model.py:265-362): class-mean prototypes of the support
// features and the Euclidean distances + softmax(-distances) of the query features against them.  The prototype MLP
// between the two (Linear, ReLU, Linear) stays on the row linear (mmfusion.ops).  At the reference's episode sizes
// (n_way = 7, n_shot <= 50, Nq = 16, d = 512) these are a few hundred KB and latency-bound: each op is one launch,
// f32 arithmetic, wave64 reductions, and every output element has exactly one writer (no atomics: eager and replayed
// runs are bit-identical).
#include "mmf_internal.h"

namespace {

constexpr int FS_THREADS = 256;
constexpr int FS_WAVES = FS_THREADS / 64;
constexpr int FS_MAXD = 1024;
constexpr int FS_MAXWAY = 64;                  // one wave holds a query's n_way distances (= mmf_fusion_loss's C limit)
constexpr int FS_MAXSHOT = 64;
constexpr int FS_MAXQ = 1024;

__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 sum3(const float4 t, const float4 a, const float4 v) {
  return make_float4((t.x + a.x) + v.x, (t.y + a.y) + v.y, (t.z + a.z) + v.z, (t.w + a.w) + v.w);   // the reference's order
}

// support_features[r] = (t + a) + v for every row r = c * n_shot + s (class-major), mean[c] = sum_s row / n_shot.
// One thread per (class, 4 columns): the shots are summed in order, in f32.
__global__ __launch_bounds__(FS_THREADS)
void proto_fwd_kernel(const float* t, const float* a, const float* v, float* sf, float* mean, int n_way, int n_shot, int d) {
  const int d4 = d >> 2;
  const int idx = blockIdx.x * FS_THREADS + threadIdx.x;
  if (idx >= n_way * d4) return;
  const int c = idx / d4, k = (idx - c * d4) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < n_shot; ++s) {
    const size_t o = ((size_t)c * n_shot + s) * d + k;
    const float4 x = sum3(ld4(t + o), ld4(a + o), ld4(v + o));
    st4(sf + o, x);
    acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
  }
  const float n = (float)n_shot;
  st4(mean + (size_t)c * d + k, make_float4(acc.x / n, acc.y / n, acc.z / n, acc.w / n));
}

// dS[r] = dmean[c] / n_shot + dsf[r] (dsf may be null): the one gradient of the three modality inputs.
__global__ __launch_bounds__(FS_THREADS)
void proto_bwd_kernel(const float* dmean, const float* dsf, float* ds, int n_way, int n_shot, int d) {
  const int d4 = d >> 2;
  const int idx = blockIdx.x * FS_THREADS + threadIdx.x;
  if (idx >= n_way * n_shot * d4) return;
  const int r = idx / d4, k = (idx - r * d4) * 4, c = r / n_shot;
  const float n = (float)n_shot;
  const float4 g = ld4(dmean + (size_t)c * d + k);
  float4 y = make_float4(g.x / n, g.y / n, g.z / n, g.w / n);
  if (dsf) {
    const float4 u = ld4(dsf + (size_t)r * d + k);
    y.x += u.x; y.y += u.y; y.z += u.z; y.w += u.w;
  }
  st4(ds + (size_t)r * d + k, y);
}

// One workgroup per query row i: q = (t + a) + v (kept in LDS, written as query_features), then wave w takes the
// prototypes j = w, w + 4, ...: dist[i][j] = sqrt(sum_k (q_k - p_jk)^2) (direct differences, float4 per lane, wave64
// sum), then wave 0 forms pred[i] = softmax(-dist[i]) with one lane per prototype.
__global__ __launch_bounds__(FS_THREADS)
void dist_fwd_kernel(const float* t, const float* a, const float* v, const float* P, float* qf, float* dist, float* pred,
                     int n_way, int d) {
  __shared__ float q_s[FS_MAXD];
  __shared__ float dist_s[FS_MAXWAY];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = 4 * tid; k < d; k += 4 * FS_THREADS) {
    const size_t o = (size_t)i * d + k;
    const float4 x = sum3(ld4(t + o), ld4(a + o), ld4(v + o));
    st4(q_s + k, x);
    st4(qf + o, x);
  }
  __syncthreads();
  for (int j = wave; j < n_way; j += FS_WAVES) {
    float s = 0.f;
    for (int k = 4 * lane; k < d; k += 4 * 64) {
      const float4 p = ld4(P + (size_t)j * d + k);
      const float e0 = q_s[k] - p.x, e1 = q_s[k + 1] - p.y, e2 = q_s[k + 2] - p.z, e3 = q_s[k + 3] - p.w;
      s += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
    }
    s = wave_sum(s);
    if (lane == 0) {
      const float r = sqrtf(s);
      dist_s[j] = r;
      dist[(size_t)i * n_way + j] = r;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const bool on = lane < n_way;
    const float x = on ? -dist_s[lane] : -INFINITY;
    const float m = wave_max(x);
    const float e = on ? expf(x - m) : 0.f;
    const float sum = wave_sum(e);
    if (on) pred[(size_t)i * n_way + lane] = e / sum;
  }
}

// c_ij = dL/ddist_ij / dist_ij (0 where dist_ij = 0: torch's cdist backward) for the lane-th prototype of row i, with
// dL/ddist_ij = gdist_ij - pred_ij (gpred_ij - sum_k pred_ik gpred_ik) (softmax(-dist) backward).  Called by a whole
// wave; lane j < n_way gets c_ij.  Both workgroup kinds of dist_bwd_kernel compute c the same way, bit for bit.
__device__ __forceinline__ float dist_coef(const float* dist, const float* pred, const float* gdist, const float* gpred,
                                           int i, int n_way, int lane) {
  const bool on = lane < n_way;
  const size_t o = (size_t)i * n_way + lane;
  float g = 0.f;
  if (gpred) {
    const float p = on ? pred[o] : 0.f;
    const float gp = on ? gpred[o] : 0.f;
    const float s = wave_sum(p * gp);
    g = -p * (gp - s);
  }
  if (!on) return 0.f;
  if (gdist) g += gdist[o];
  const float r = dist[o];
  return r > 0.f ? g / r : 0.f;
}

// Workgroups [0, Nq): dq[i] = sum_j c_ij (q_i - p_j).  Workgroups [Nq, Nq + n_way): dp[j] = -sum_i c_ij (q_i - p_j).
// Each first gathers its c row / column into LDS, then one thread per 4 columns sums over j (or i) in order.
__global__ __launch_bounds__(FS_THREADS)
void dist_bwd_kernel(const float* qf, const float* P, const float* dist, const float* pred, const float* gdist,
                     const float* gpred, float* dq, float* dp, int Nq, int n_way, int d) {
  __shared__ float c_s[FS_MAXQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x < Nq) {
    if (!dq) return;
    const int i = blockIdx.x;
    if (wave == 0) {
      const float c = dist_coef(dist, pred, gdist, gpred, i, n_way, lane);
      if (lane < n_way) c_s[lane] = c;
    }
    __syncthreads();
    for (int k = 4 * tid; k < d; k += 4 * FS_THREADS) {
      const float4 q = ld4(qf + (size_t)i * d + k);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int j = 0; j < n_way; ++j) {
        const float c = c_s[j];
        const float4 p = ld4(P + (size_t)j * d + k);
        acc.x += c * (q.x - p.x); acc.y += c * (q.y - p.y); acc.z += c * (q.z - p.z); acc.w += c * (q.w - p.w);
      }
      st4(dq + (size_t)i * d + k, acc);
    }
  } else {
    if (!dp) return;
    const int j = blockIdx.x - Nq;
    for (int i = wave; i < Nq; i += FS_WAVES) {
      const float c = dist_coef(dist, pred, gdist, gpred, i, n_way, lane);
      if (lane == j) c_s[i] = c;
    }
    __syncthreads();
    for (int k = 4 * tid; k < d; k += 4 * FS_THREADS) {
      const float4 p = ld4(P + (size_t)j * d + k);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 0; i < Nq; ++i) {
        const float c = c_s[i];
        const float4 q = ld4(qf + (size_t)i * d + k);
        acc.x += c * (q.x - p.x); acc.y += c * (q.y - p.y); acc.z += c * (q.z - p.z); acc.w += c * (q.w - p.w);
      }
      st4(dp + (size_t)j * d + k, make_float4(-acc.x, -acc.y, -acc.z, -acc.w));
    }
  }
}

int check_dims(const char* who, int n_way, int n_shot, int Nq, int d) {
  if (d <= 0 || d > FS_MAXD || d % 4 || n_way < 1 || n_way > FS_MAXWAY || n_shot < 1 || n_shot > FS_MAXSHOT || Nq < 1 ||
      Nq > FS_MAXQ)
    MMF_FAIL(MMF_E_SHAPE, "%s: d=%d (multiple of 4, <= %d) n_way=%d (1..%d) n_shot=%d (1..%d) Nq=%d (1..%d)", who, d, FS_MAXD,
             n_way, FS_MAXWAY, n_shot, FS_MAXSHOT, Nq, FS_MAXQ);
  return MMF_OK;
}

int check_ptrs(const char* who, std::initializer_list<const void*> need, std::initializer_list<const void*> vec) {
  for (const void* p : need)
    if (!p) MMF_FAIL(MMF_E_SHAPE, "%s: null operand or output", who);
  for (const void* p : vec)
    if (p && !mmf_aligned16(p)) MMF_FAIL(MMF_E_ALIGN, "%s: a feature-row operand is not 16-byte aligned", who);
  return MMF_OK;
}

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + FS_THREADS - 1) / FS_THREADS); }

}  // namespace

extern "C" int mmf_fewshot_proto_fwd(const float* const s[3], float* sf, float* mean, int n_way, int n_shot, int d,
                                     void* stream) {
  const char* who = "mmf_fewshot_proto_fwd";
  int rc = check_dims(who, n_way, n_shot, 1, d);
  if (rc != MMF_OK) return rc;
  if (!s) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", who);
  rc = check_ptrs(who, {s[0], s[1], s[2], sf, mean}, {s[0], s[1], s[2], sf, mean});
  if (rc != MMF_OK) return rc;
  hipLaunchKernelGGL(proto_fwd_kernel, dim3(blocks_for((size_t)n_way * (d / 4))), dim3(FS_THREADS), 0,
                     static_cast<hipStream_t>(stream), s[0], s[1], s[2], sf, mean, n_way, n_shot, d);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}

extern "C" int mmf_fewshot_proto_bwd(const float* dmean, const float* dsf, float* ds, int n_way, int n_shot, int d,
                                     void* stream) {
  const char* who = "mmf_fewshot_proto_bwd";
  int rc = check_dims(who, n_way, n_shot, 1, d);
  if (rc != MMF_OK) return rc;
  rc = check_ptrs(who, {dmean, ds}, {dmean, dsf, ds});
  if (rc != MMF_OK) return rc;
  hipLaunchKernelGGL(proto_bwd_kernel, dim3(blocks_for((size_t)n_way * n_shot * (d / 4))), dim3(FS_THREADS), 0,
                     static_cast<hipStream_t>(stream), dmean, dsf, ds, n_way, n_shot, d);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}

extern "C" int mmf_fewshot_dist_fwd(const float* const q[3], const float* P, float* qf, float* dist, float* pred, int Nq,
                                    int n_way, int d, void* stream) {
  const char* who = "mmf_fewshot_dist_fwd";
  int rc = check_dims(who, n_way, 1, Nq, d);
  if (rc != MMF_OK) return rc;
  if (!q) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", who);
  rc = check_ptrs(who, {q[0], q[1], q[2], P, qf, dist, pred}, {q[0], q[1], q[2], P, qf});
  if (rc != MMF_OK) return rc;
  hipLaunchKernelGGL(dist_fwd_kernel, dim3(Nq), dim3(FS_THREADS), 0, static_cast<hipStream_t>(stream), q[0], q[1], q[2], P,
                     qf, dist, pred, n_way, d);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}

extern "C" int mmf_fewshot_dist_bwd(const float* qf, const float* P, const float* dist, const float* pred, const float* gdist,
                                    const float* gpred, float* dq, float* dp, int Nq, int n_way, int d, void* stream) {
  const char* who = "mmf_fewshot_dist_bwd";
  int rc = check_dims(who, n_way, 1, Nq, d);
  if (rc != MMF_OK) return rc;
  rc = check_ptrs(who, {qf, P, dist, pred}, {qf, P, dq, dp});
  if (rc != MMF_OK) return rc;
  if (!dq && !dp) return MMF_OK;                 // nothing wanted
  hipLaunchKernelGGL(dist_bwd_kernel, dim3(Nq + n_way), dim3(FS_THREADS), 0, static_cast<hipStream_t>(stream), qf, P, dist,
                     pred, gdist, gpred, dq, dp, Nq, n_way, d);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}
