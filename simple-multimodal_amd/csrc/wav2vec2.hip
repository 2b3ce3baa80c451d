// The pieces a Wav2Vec2 forward has and the fusion path did not (mmfusion/wav2vec2.py).  Activations are channel-last
// (time, channels) bf16 everywhere, so a convolution over time is a GEMM over a window form and the transformer needs no
// transpose.
//   conv0_stats / conv0_norm_gelu   layer 0: Conv1d(1 -> C0, k0, s0) + GroupNorm(one group per channel) + GELU in two passes
//                                   that both recompute the k0 MACs per output; no f32 intermediate is stored
//   gelu_window                     GELU + the (T_out, k*C) window form the next conv layer's GEMM reads
//   posconv                         the grouped positional convolution as one MFMA GEMM per (clip, group, 128 time rows)
#include "mmf_internal.h"

namespace {

constexpr int W2V_THREADS = 256;
constexpr int W2V_SLOTS = MMF_W2V_STATS_SLOTS;      // frame lanes per clip in the statistics pass


// ---- layer 0 -------------------------------------------------------------------------------------------
// A thread owns 8 consecutive channels (their K0 taps stay in registers) and walks frames; the C0 / 8 threads of one frame
// sit next to each other, so every store of a frame row is contiguous and the waveform loads are broadcasts.
// K0 is the register tap count: taps k0 .. K0 - 1 are zero.
template <int K0>
struct Conv0 {
  float w[8][K0];
  __device__ __forceinline__ void load(const float* __restrict__ wt, int c, int k0) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int j = 0; j < K0; ++j) w[e][j] = j < k0 ? wt[(size_t)(c + e) * k0 + j] : 0.0f;
  }
  __device__ __forceinline__ void frame(const float* __restrict__ xs, int k0, float* v) const {
    float x[K0];
#pragma unroll
    for (int j = 0; j < K0; ++j) x[j] = j < k0 ? xs[j] : 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = 0.0f;
#pragma unroll
      for (int j = 0; j < K0; ++j) a = fmaf(w[e][j], x[j], a);
      v[e] = a;
    }
  }
};

// pass 1a: Welford mean / M2 of this thread's frames f = slot, slot + nslots, ... -> partial[clip][slot][mean | M2][C0]
template <int K0>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_partial_kernel(const float* __restrict__ wave, const float* __restrict__ wt, float* __restrict__ partial,
                              int L, int T0, int C0, int k0, int s0, int nfl, int cgn) {
  const int cgi = threadIdx.x % cgn, fl = threadIdx.x / cgn;
  if (fl >= nfl) return;
  const int slot = blockIdx.x * nfl + fl, nslots = gridDim.x * nfl, c = cgi * 8;
  Conv0<K0> cv;
  cv.load(wt, c, k0);
  const float* __restrict__ xs = wave + (size_t)blockIdx.y * L;
  float mean[8], m2[8], v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mean[e] = m2[e] = 0.0f;
  int cnt = 0;
  for (int f = slot; f < T0; f += nslots) {
    cv.frame(xs + (size_t)f * s0, k0, v);
    const float inv = 1.0f / (float)(++cnt);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = v[e] - mean[e];
      mean[e] += d * inv;
      m2[e] = fmaf(d, v[e] - mean[e], m2[e]);
    }
  }
  float* __restrict__ p = partial + (((size_t)blockIdx.y * W2V_SLOTS + slot) * 2) * C0 + c;
  *reinterpret_cast<f32x4_t*>(p) = f32x4_t{mean[0], mean[1], mean[2], mean[3]};
  *reinterpret_cast<f32x4_t*>(p + 4) = f32x4_t{mean[4], mean[5], mean[6], mean[7]};
  *reinterpret_cast<f32x4_t*>(p + C0) = f32x4_t{m2[0], m2[1], m2[2], m2[3]};
  *reinterpret_cast<f32x4_t*>(p + C0 + 4) = f32x4_t{m2[4], m2[5], m2[6], m2[7]};
}

// pass 1b: merge the slots of one (clip, channel) in slot order (Chan's update) -> stats[clip][mean | biased variance][C0]
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_merge_kernel(const float* __restrict__ partial, float* __restrict__ stats, int T0, int C0, int nslots) {
  const int c = blockIdx.x * W2V_THREADS + threadIdx.x;
  if (c >= C0) return;
  const float* __restrict__ p = partial + (size_t)blockIdx.y * W2V_SLOTS * 2 * C0 + c;
  float n = 0.0f, mean = 0.0f, m2 = 0.0f;
  for (int s = 0; s < nslots && s < T0; ++s) {
    const float nb = (float)((T0 - s + nslots - 1) / nslots);
    const float mb = p[(size_t)s * 2 * C0], qb = p[(size_t)s * 2 * C0 + C0];
    const float nn = n + nb, d = mb - mean;
    mean += d * (nb / nn);
    m2 += qb + d * d * (n * nb / nn);
    n = nn;
  }
  stats[(size_t)blockIdx.y * 2 * C0 + c] = mean;
  stats[(size_t)blockIdx.y * 2 * C0 + C0 + c] = m2 / n;
}

// pass 2: recompute, normalise, GELU, and store frame f at every (row t1, tap j) of the next layer's window form with
// s1 * t1 + j == f: out[clip][t1][j * C0 + c]
template <int K0>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_norm_gelu_kernel(const float* __restrict__ wave, const float* __restrict__ wt, const float* __restrict__ stats,
                                const float* __restrict__ gamma, const float* __restrict__ beta, unsigned short* __restrict__ out,
                                int L, int T0, int C0, int k0, int s0, int k1, int s1, int T1, float eps, int nfl, int cgn) {
  const int cgi = threadIdx.x % cgn, fl = threadIdx.x / cgn;
  if (fl >= nfl) return;
  const int c = cgi * 8;
  Conv0<K0> cv;
  cv.load(wt, c, k0);
  float scale[8], shift[8], v[8];
  const float* __restrict__ st = stats + (size_t)blockIdx.y * 2 * C0 + c;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    scale[e] = gamma[c + e] * rsqrtf(st[C0 + e] + eps);
    shift[e] = beta[c + e] - st[e] * scale[e];
  }
  const float* __restrict__ xs = wave + (size_t)blockIdx.y * L;
  unsigned short* __restrict__ dst = out + (size_t)blockIdx.y * T1 * k1 * C0 + c;
  const int last = s1 * (T1 - 1) + k1 - 1;                 // the last frame the next layer reads
  for (int f = blockIdx.x * nfl + fl; f <= last; f += gridDim.x * nfl) {
    cv.frame(xs + (size_t)f * s0, k0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = gelu_erf(fmaf(v[e], scale[e], shift[e]));
    const u32x4_t pk = pack8(v);
    for (int j = 0; j < k1 && j <= f; ++j) {
      const int t1 = (f - j) / s1;
      if (t1 * s1 == f - j && t1 < T1) *reinterpret_cast<u32x4_t*>(dst + ((size_t)t1 * k1 + j) * C0) = pk;
    }
  }
}

// ---- GELU + window form ------------------------------------------------------------------------------------
// x (T_in, C) raw conv output per clip -> out (T_out, k*C): out[t][j*C + c] = gelu(x[s*t + j][c]).  The lanes walk the OUTPUT in
// order; a lane's 8 columns are 8 consecutive channels of one input row.
__global__ __launch_bounds__(W2V_THREADS)
void w2v_gelu_window_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ out, int T_in, int C, int k, int s,
                            unsigned cv /* C/8 */, unsigned nvec /* T_out*k*C/8 */) {
  const unsigned short* __restrict__ src = x + (size_t)blockIdx.y * T_in * C;
  unsigned short* __restrict__ dst = out + (size_t)blockIdx.y * nvec * 8;
  const unsigned rowv = cv * (unsigned)k, stride = gridDim.x * W2V_THREADS;
  for (unsigned v = blockIdx.x * W2V_THREADS + threadIdx.x; v < nvec; v += stride) {
    const unsigned t = v / rowv, r = v - t * rowv;
    const unsigned j = r / cv, c = (r - j * cv) << 3;
    float a[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(src + ((size_t)t * s + j) * C + c), a);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = gelu_erf(a[e]);
    *reinterpret_cast<u32x4_t*>(dst + (size_t)v * 8) = pack8(a);
  }
}

// ---- positional convolution -------------------------------------------------------------------------------
// y[t][g*CG + co] = x[t][g*CG + co] + gelu(b[g*CG + co] + sum_{j < k, ci < CG} w[g][co][j*CG + ci] * x[t + j - k/2][g*CG + ci]),
// rows outside [0, T) read as zero.  One workgroup = (128 time rows, group, clip).  The group's channels of rows
// [t0 - k/2, t0 + 127 + k - 1 - k/2] are staged in LDS as (rows, CG) with row stride CG, so the k*CG inputs of output row r are
// the contiguous span at r*CG: a GEMM with K = k*CG whose B operand (v_mfma_f32_16x16x32_bf16: B[k][col = time]) is one
// ds_read_b128 per lane and step, and whose A operand (A[row = co][k]) streams from the repacked weights in L2.  Kp = k*CG
// rounded up to 32: the weight rows are zero-padded and so is the tail of the LDS image.
// LDS banks: a 16-lane ds_read_b128 group reads 16 rows x one 16-byte quarter; with CG = 48 the row stride is 24 banks and the
// 16 slots start at 16 different multiples of 4 banks (24 r mod 64 takes 8 values, the two quarters of a group differ by 4):
// conflict-free.  CG = 32 and 64 (row stride 16 / 32 banks) are 4-way conflicted; no shipped model has them.
// D[row = co = 4 (lane >> 4) + reg][col = time = lane & 15]: a lane ends with 4 consecutive channels of one time row.
template <int CT>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_posconv_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ wp, const float* __restrict__ bias,
                        unsigned short* __restrict__ y, int T, int C, int k, int Kp) {
  constexpr int CG = CT * 16, TT = 128;
  extern __shared__ __attribute__((aligned(16))) unsigned short sx[];
  const int t0 = blockIdx.x * TT, g = blockIdx.y, pad = k >> 1;
  const unsigned short* __restrict__ xn = x + (size_t)blockIdx.z * T * C + g * CG;
  const int nvec = ((TT - 1) * CG + Kp) >> 3, rows = TT + k - 1;
  for (int v = threadIdx.x; v < nvec; v += W2V_THREADS) {
    const int e = v << 3, rr = e / CG, cc = e - rr * CG, t = t0 - pad + rr;
    u32x4_t val = {0u, 0u, 0u, 0u};
    if (rr < rows && t >= 0 && t < T) val = *reinterpret_cast<const u32x4_t*>(xn + (size_t)t * C + cc);
    *reinterpret_cast<u32x4_t*>(sx + e) = val;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int tw = t0 + wave * 32;                                   // this wave's 32 time rows
  if (tw >= T) return;
  f32x4_t acc[2][CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[0][ct] = acc[1][ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const unsigned short* __restrict__ wg = wp + ((size_t)g * CG + r) * Kp + q * 8;
  const unsigned short* sb = sx + (wave * 32 + r) * CG + q * 8;
  const int steps = Kp >> 5;
  for (int ks = 0; ks < steps; ++ks) {
    const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(sb + ks * 32);
    const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(sb + 16 * CG + ks * 32);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(wg + (size_t)ct * 16 * Kp + ks * 32);
      acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[0][ct], 0, 0, 0);
      acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[1][ct], 0, 0, 0);
    }
  }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int t = tw + tt * 16 + r;
    if (t >= T) continue;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int co = ct * 16 + q * 4;
      const f32x4_t b = *reinterpret_cast<const f32x4_t*>(bias + g * CG + co);
      const u32x2_t xr = *reinterpret_cast<const u32x2_t*>(xn + (size_t)t * C + co);
      const f32x4_t a = acc[tt][ct] + b;
      const u32x2_t o = {pack_bf16x2(bf16lo(xr[0]) + gelu_erf(a[0]), bf16hi(xr[0]) + gelu_erf(a[1])),
                         pack_bf16x2(bf16lo(xr[1]) + gelu_erf(a[2]), bf16hi(xr[1]) + gelu_erf(a[3]))};
      *reinterpret_cast<u32x2_t*>(y + ((size_t)blockIdx.z * T + t) * C + g * CG + co) = o;
    }
  }
}

struct Conv0Shape { int T0, T1, cgn, nfl, nblk; };

// shared validation of the two layer-0 entry points; T1 is only meaningful with k1 > 0
int conv0_check(const char* fn, int N, int L, int C0, int k0, int s0, Conv0Shape* sh) {
  if (N <= 0 || L <= 0 || C0 <= 0 || k0 <= 0 || s0 <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: N=%d L=%d C0=%d k0=%d s0=%d", fn, N, L, C0, k0, s0);
  if (L < k0) MMF_FAIL(MMF_E_SHAPE, "%s: L=%d is shorter than the kernel k0=%d", fn, L, k0);
  if ((C0 & 7) || C0 > 2048 || k0 > 16 || N > 65535)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: C0=%d (multiple of 8, at most 2048), k0=%d (at most 16), N=%d (at most 65535)", fn, C0, k0, N);
  sh->T0 = (L - k0) / s0 + 1;
  sh->cgn = C0 / 8;
  sh->nfl = W2V_THREADS / sh->cgn > 32 ? 32 : W2V_THREADS / sh->cgn;      // frames per workgroup pass
  sh->nblk = W2V_SLOTS / sh->nfl;
  if (sh->nblk < 1) sh->nblk = 1;
  return MMF_OK;
}

}  // namespace

extern "C" int mmf_w2v_conv0_stats(const float* wave, const float* weight, float* stats, float* partial, int N, int L, int C0,
                                   int k0, int s0, void* stream) {
  if (!wave || !weight || !stats || !partial) MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_conv0_stats: null operand");
  Conv0Shape sh;
  if (int rc = conv0_check("mmf_w2v_conv0_stats", N, L, C0, k0, s0, &sh)) return rc;
  if (!mmf_aligned16(stats) || !mmf_aligned16(partial) || (reinterpret_cast<uintptr_t>(wave) & 3u) || (reinterpret_cast<uintptr_t>(weight) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "mmf_w2v_conv0_stats: stats / partial must be 16-byte aligned, wave / weight 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int nblk = sh.nblk;
  if ((int64_t)nblk * sh.nfl > sh.T0) nblk = (sh.T0 + sh.nfl - 1) / sh.nfl;
  const int nslots = nblk * sh.nfl;                                       // <= MMF_W2V_STATS_SLOTS
  if (k0 <= 10) hipLaunchKernelGGL(w2v_conv0_partial_kernel<10>, dim3(nblk, N), dim3(W2V_THREADS), 0, s, wave, weight, partial, L, sh.T0, C0, k0, s0, sh.nfl, sh.cgn);
  else          hipLaunchKernelGGL(w2v_conv0_partial_kernel<16>, dim3(nblk, N), dim3(W2V_THREADS), 0, s, wave, weight, partial, L, sh.T0, C0, k0, s0, sh.nfl, sh.cgn);
  MMF_CHECK_LAUNCH("mmf_w2v_conv0_stats");
  hipLaunchKernelGGL(w2v_conv0_merge_kernel, dim3((C0 + W2V_THREADS - 1) / W2V_THREADS, N), dim3(W2V_THREADS), 0, s, partial, stats, sh.T0, C0, nslots);
  MMF_CHECK_LAUNCH("mmf_w2v_conv0_stats");
  return MMF_OK;
}

extern "C" int mmf_w2v_conv0_norm_gelu(const float* wave, const float* weight, const float* stats, const float* gamma,
                                       const float* beta, void* out_bf16, int N, int L, int C0, int k0, int s0, int k1, int s1,
                                       float eps, void* stream) {
  if (!wave || !weight || !stats || !gamma || !beta || !out_bf16) MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_conv0_norm_gelu: null operand");
  Conv0Shape sh;
  if (int rc = conv0_check("mmf_w2v_conv0_norm_gelu", N, L, C0, k0, s0, &sh)) return rc;
  if (k1 <= 0 || s1 <= 0 || sh.T0 < k1) MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_conv0_norm_gelu: k1=%d s1=%d against T0=%d frames", k1, s1, sh.T0);
  if (!mmf_aligned16(out_bf16) || !mmf_aligned16(stats) || (reinterpret_cast<uintptr_t>(wave) & 3u) || (reinterpret_cast<uintptr_t>(weight) & 3u)
      || (reinterpret_cast<uintptr_t>(gamma) & 3u) || (reinterpret_cast<uintptr_t>(beta) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "mmf_w2v_conv0_norm_gelu: out / stats must be 16-byte aligned, the f32 operands 4-byte aligned");
  const int T1 = (sh.T0 - k1) / s1 + 1;
  int64_t blocks = ((int64_t)sh.T0 + sh.nfl - 1) / sh.nfl;
  if (blocks > 1024) blocks = 1024;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned short* out = static_cast<unsigned short*>(out_bf16);
  if (k0 <= 10) hipLaunchKernelGGL(w2v_conv0_norm_gelu_kernel<10>, dim3((int)blocks, N), dim3(W2V_THREADS), 0, s, wave, weight, stats, gamma, beta, out, L, sh.T0, C0, k0, s0, k1, s1, T1, eps, sh.nfl, sh.cgn);
  else          hipLaunchKernelGGL(w2v_conv0_norm_gelu_kernel<16>, dim3((int)blocks, N), dim3(W2V_THREADS), 0, s, wave, weight, stats, gamma, beta, out, L, sh.T0, C0, k0, s0, k1, s1, T1, eps, sh.nfl, sh.cgn);
  MMF_CHECK_LAUNCH("mmf_w2v_conv0_norm_gelu");
  return MMF_OK;
}

extern "C" int mmf_w2v_gelu_window(const void* x_bf16, void* out_bf16, int N, int T_in, int C, int k, int s, void* stream) {
  if (!x_bf16 || !out_bf16 || N <= 0 || T_in <= 0 || C <= 0 || k <= 0 || s <= 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_gelu_window: null operand or N=%d T_in=%d C=%d k=%d s=%d", N, T_in, C, k, s);
  if (T_in < k) MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_gelu_window: T_in=%d is shorter than the kernel k=%d", T_in, k);
  const int64_t T_out = (T_in - k) / s + 1, nvec = T_out * k * (C / 8);
  if ((C & 7) || N > 65535 || nvec >= (int64_t)1 << 31 || x_bf16 == out_bf16)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_w2v_gelu_window: C=%d (multiple of 8), N=%d (at most 65535), %lld output elements per clip (below 2^34), "
             "out must not be x", C, N, (long long)nvec * 8);
  if (!mmf_aligned16(x_bf16) || !mmf_aligned16(out_bf16)) MMF_FAIL(MMF_E_ALIGN, "mmf_w2v_gelu_window: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(w2v_gelu_window_kernel, dim3(mmf_stream_grid(nvec, W2V_THREADS), N), dim3(W2V_THREADS), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(x_bf16), static_cast<unsigned short*>(out_bf16), T_in, C, k, s, (unsigned)(C / 8), (unsigned)nvec);
  MMF_CHECK_LAUNCH("mmf_w2v_gelu_window");
  return MMF_OK;
}

extern "C" int mmf_w2v_posconv(const void* x_bf16, const void* w_bf16, const float* bias, void* y_bf16, int N, int T, int C,
                               int groups, int k, void* stream) {
  if (!x_bf16 || !w_bf16 || !bias || !y_bf16 || N <= 0 || T <= 0 || C <= 0 || groups <= 0 || k <= 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_posconv: null operand or N=%d T=%d C=%d groups=%d k=%d", N, T, C, groups, k);
  if (C % groups) MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_posconv: C=%d is not a multiple of groups=%d", C, groups);
  const int cg = C / groups;
  if ((cg & 15) || cg > 64 || N > 65535 || groups > 65535 || x_bf16 == y_bf16)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_w2v_posconv: group width %d (16, 32, 48 or 64), N=%d groups=%d (at most 65535), y must not be x", cg, N, groups);
  const int Kp = (k * cg + 31) & ~31;
  const size_t lds = ((size_t)127 * cg + Kp) * 2;
  if (lds > 65536) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_w2v_posconv: k=%d at group width %d needs %zu bytes of LDS (at most 65536)", k, cg, lds);
  if (!mmf_aligned16(x_bf16) || !mmf_aligned16(w_bf16) || !mmf_aligned16(bias) || !mmf_aligned16(y_bf16))
    MMF_FAIL(MMF_E_ALIGN, "mmf_w2v_posconv: pointers must be 16-byte aligned");
  const dim3 grid((T + 127) / 128, groups, N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned short* x = static_cast<const unsigned short*>(x_bf16);
  const unsigned short* w = static_cast<const unsigned short*>(w_bf16);
  unsigned short* y = static_cast<unsigned short*>(y_bf16);
  switch (cg / 16) {
    case 1: hipLaunchKernelGGL(w2v_posconv_kernel<1>, grid, dim3(W2V_THREADS), lds, s, x, w, bias, y, T, C, k, Kp); break;
    case 2: hipLaunchKernelGGL(w2v_posconv_kernel<2>, grid, dim3(W2V_THREADS), lds, s, x, w, bias, y, T, C, k, Kp); break;
    case 3: hipLaunchKernelGGL(w2v_posconv_kernel<3>, grid, dim3(W2V_THREADS), lds, s, x, w, bias, y, T, C, k, Kp); break;
    default: hipLaunchKernelGGL(w2v_posconv_kernel<4>, grid, dim3(W2V_THREADS), lds, s, x, w, bias, y, T, C, k, Kp); break;
  }
  MMF_CHECK_LAUNCH("mmf_w2v_posconv");
  return MMF_OK;
}
