// The pieces a Wav2Vec2 forward has and the fusion path did not (mmfusion/wav2vec2.py).  Activations are channel-last
// (time, channels) bf16 everywhere, so a convolution over time is a GEMM over a window form and the transformer needs no
// transpose.
//   conv0_stats / conv0_norm_gelu   layer 0: Conv1d(1 -> C0, k0, s0) + GroupNorm(one group per channel) + GELU in two passes
//                                   that both recompute the k0 MACs per output; no f32 intermediate is stored
//   gelu_window                     GELU + the (T_out, k*C) window form the next conv layer's GEMM reads
//   conv0_ln_gelu / ln_gelu_window  the layer-norm family's forms of the two: LayerNorm over the channels of every frame (with conv
//                                   biases) in front of the GELU, the frame's statistics reduced across the C / 8 lanes that own it
//   window_fold_gelu_bwd            its mirror: the gradient of the window form gathered back to the raw output's, times gelu'
//   conv0_bwd_stats / _bwd_wgrad    layer 0's backward: GroupNorm's two sums per channel, then dW0, recomputing as the forward does
//   posconv                         the grouped positional convolution as one MFMA GEMM per (clip, group, 128 time rows); the same
//                                   body with two more epilogues is its backward's dz = dy gelu'(z) and input gradient
//   posconv_wgrad                   its weight gradient: an MFMA GEMM per (group, 8 taps) whose contraction runs over time
//   weightnorm_bwd                  the effective weight's gradient -> the gradients of the weight norm's g and v
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

// ---- the layer-norm family: LayerNorm over the channels of a frame ------------------------------------------------
// The C / 8 lanes that own a frame sit next to each other (cgn = C / 8, a power of two up to 256).  row_sum adds one value per lane
// over them: xor-shuffles inside a wave (cgn <= 64: the partners of a lane are the lanes of its own frame), and for a frame that
// spans 2 or 4 waves the waves' sums go through `red` (one row of W2V_THREADS / 64 floats per call site, so that two reductions
// of one loop pass need one barrier each) and are added in wave order.  Every lane of the workgroup must call it: the callers'
// loops have workgroup-uniform trip counts and predicate their stores instead of branching around it.
__device__ __forceinline__ float w2v_row_sum(float v, int cgn, float* red) {
  if (cgn <= 64) {
    for (int o = cgn >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, wpr = cgn >> 6, w0 = wave / wpr * wpr;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  float a = red[w0];
  for (int w = 1; w < wpr; ++w) a += red[w0 + w];
  return a;
}

// v[8] (one lane's channels of a frame of C = 8 cgn channels) -> gelu(gamma xhat + beta), the mean and then the squared deviations
// from it summed over the values in registers (two passes: no E[x^2] - mean^2)
__device__ __forceinline__ void w2v_ln_gelu8(float (&v)[8], const float (&gamma)[8], const float (&beta)[8], int cgn, float eps,
                                             float (*red)[W2V_THREADS / 64]) {
  const float inv = 1.0f / (float)(cgn * 8);
  float a = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  const float mean = w2v_row_sum(a, cgn, red[0]) * inv;
  float q = 0.0f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    v[e] -= mean;
    q = fmaf(v[e], v[e], q);
  }
  const float rstd = rsqrtf(w2v_row_sum(q, cgn, red[1]) * inv + eps);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = gelu_erf(fmaf(v[e] * rstd, gamma[e], beta[e]));
}

// frame f, 8 channels as pk, to every (row t, tap j) of the window form with s t + j == f: dst[(t k + j) C] (dst: the clip's window
// form at this lane's channel)
__device__ __forceinline__ void w2v_scatter8(unsigned short* __restrict__ dst, const u32x4_t pk, int f, int C, int k, int s, int T_out) {
  for (int j = 0; j < k && j <= f; ++j) {
    const int t = (f - j) / s;
    if (t * s == f - j && t < T_out) *reinterpret_cast<u32x4_t*>(dst + ((size_t)t * k + j) * C) = pk;
  }
}

// Layer 0 in one pass: conv + bias, LayerNorm over the C0 channels of the frame, GELU, one rounding, the window form of layer 1
// (w2v_conv0_norm_gelu_kernel's scatter).  nfl = W2V_THREADS / cgn frames per workgroup pass; a lane past the last frame layer 1
// reads computes that last frame again and stores nothing.
template <int K0>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_ln_gelu_kernel(const float* __restrict__ wave, const float* __restrict__ wt, const float* __restrict__ bias,
                              const float* __restrict__ gamma, const float* __restrict__ beta, unsigned short* __restrict__ out,
                              int L, int C0, int k0, int s0, int k1, int s1, int T1, float eps, int nfl, int cgn) {
  __shared__ float red[2][W2V_THREADS / 64];
  const int cgi = threadIdx.x % cgn, fl = threadIdx.x / cgn, c = cgi * 8;
  Conv0<K0> cv;
  cv.load(wt, c, k0);
  float b[8], ga[8], be[8], v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    b[e] = bias ? bias[c + e] : 0.0f;
    ga[e] = gamma[c + e];
    be[e] = beta[c + e];
  }
  const float* __restrict__ xs = wave + (size_t)blockIdx.y * L;
  unsigned short* __restrict__ dst = out + (size_t)blockIdx.y * T1 * k1 * C0 + c;
  const int last = s1 * (T1 - 1) + k1 - 1;                 // the last frame the next layer reads
  for (int f0 = blockIdx.x * nfl; f0 <= last; f0 += gridDim.x * nfl) {
    const int f = f0 + fl;
    const bool live = f <= last;
    cv.frame(xs + (size_t)(live ? f : last) * s0, k0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += b[e];
    w2v_ln_gelu8(v, ga, be, cgn, eps, red);
    if (live) w2v_scatter8(dst, pack8(v), f, C0, k1, s1, T1);
  }
}

// The inner layers: x (T_in, C) raw conv output (bias added) per clip -> out[t][j*C + c] = gelu(LN(x[s t + j])[c]).  The lanes walk
// the INPUT rows, rpb = W2V_THREADS / cgn of them per workgroup pass: a row is normalised once and stored to every slot that reads
// it.  k = 0: out is (T_in, C) and may be x (a row's lanes have all read it, and been through a reduction, before one of them writes;
// a lane past the end reads nothing and normalises zeros).  T_read: the rows some window reads (all of them for k = 0); the rest are skipped.
__global__ __launch_bounds__(W2V_THREADS)
void w2v_ln_gelu_window_kernel(const unsigned short* x, const float* __restrict__ gamma, const float* __restrict__ beta,
                               unsigned short* out, int T_in, int T_read, int T_out, int C, int k, int s, float eps, int rpb, int cgn) {
  __shared__ float red[2][W2V_THREADS / 64];
  const int cgi = threadIdx.x % cgn, rl = threadIdx.x / cgn, c = cgi * 8;
  float ga[8], be[8], v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    ga[e] = gamma[c + e];
    be[e] = beta[c + e];
  }
  const unsigned short* src = x + (size_t)blockIdx.y * T_in * C + c;
  unsigned short* dst = out + (size_t)blockIdx.y * (k ? (size_t)T_out * k : (size_t)T_in) * C + c;
  for (int f0 = blockIdx.x * rpb; f0 < T_read; f0 += gridDim.x * rpb) {
    const int f = f0 + rl;
    const bool live = f < T_read;
    u32x4_t in = {0u, 0u, 0u, 0u};
    if (live) in = *reinterpret_cast<const u32x4_t*>(src + (size_t)f * C);
    unpack8(in, v);
    w2v_ln_gelu8(v, ga, be, cgn, eps, red);
    if (!live) continue;
    const u32x4_t pk = pack8(v);
    if (k == 0) *reinterpret_cast<u32x4_t*>(dst + (size_t)f * C) = pk;
    else w2v_scatter8(dst, pk, f, C, k, s, T_out);
  }
}

// ---- backward of the window form ---------------------------------------------------------------------------
// The fold of a window-form gradient dwin (T_out, k*C) of one clip at input frame f, channels c .. c + 7: the rows t and taps j with
// s t + j == f, j ascending (j = f % s, f % s + s, ...), added in f32 in that order.  Returns whether any window reads the frame.
__device__ __forceinline__ bool w2v_fold8(const unsigned short* __restrict__ dwin, int f, int c, int C, int k, int s, int T_out,
                                          float (&acc)[8]) {
  bool any = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
  for (int j = f % s; j < k && j <= f; j += s) {
    const int t = (f - j) / s;
    if (t >= T_out) continue;
    float a[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(dwin + ((size_t)t * k + j) * C + c), a);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += a[e];
    any = true;
  }
  return any;
}

// The mirror of w2v_gelu_window_kernel: dx[f][c] = gelu'(x[f][c]) * fold(dwin)[f][c].  The lanes walk dx in order, 8 channels each
// (a gather: no lane writes what another one does).  A frame no window reads is written as zeros.  dx may be x: a lane reads its
// own 16 bytes of x before it writes them.
__global__ __launch_bounds__(W2V_THREADS)
void w2v_window_fold_gelu_bwd_kernel(const unsigned short* __restrict__ dwin, const unsigned short* x, unsigned short* dx, int T_in,
                                     int T_out, int C, int k, int s, unsigned cv /* C/8 */, unsigned nvec /* T_in*C/8 */) {
  const unsigned short* __restrict__ g = dwin + (size_t)blockIdx.y * T_out * k * C;
  const size_t base = (size_t)blockIdx.y * nvec * 8;
  const unsigned stride = gridDim.x * W2V_THREADS;
  for (unsigned v = blockIdx.x * W2V_THREADS + threadIdx.x; v < nvec; v += stride) {
    const unsigned f = v / cv, c = (v - f * cv) << 3;
    float acc[8], a[8];
    const bool any = w2v_fold8(g, (int)f, (int)c, C, k, s, T_out, acc);
    unpack8(*reinterpret_cast<const u32x4_t*>(x + base + (size_t)v * 8), a);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = any ? acc[e] * gelu_erf_grad(a[e]) : 0.0f;
    *reinterpret_cast<u32x4_t*>(dx + base + (size_t)v * 8) = pack8(acc);
  }
}

// ---- layer 0: backward ---------------------------------------------------------------------------------------
// With c = conv0(wave), xhat = (c - mean) rstd, y = gamma xhat + beta: da0 = the fold of dwin_1 (zero on the frames layer 1 never
// reads), dy = da0 gelu'(y).  Both passes recompute c on the Conv0 body and fold dwin_1 themselves; nothing (T0, C0)-sized is stored.
template <int K0>
struct Conv0Bwd {
  Conv0<K0> cv;
  float mean[8], rstd[8], scale[8], shift[8];
  __device__ __forceinline__ void load(const float* __restrict__ wt, const float* __restrict__ st, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, int c, int C0, int k0, float eps) {
    cv.load(wt, c, k0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      mean[e] = st[e];
      rstd[e] = rsqrtf(st[C0 + e] + eps);
      scale[e] = gamma[c + e] * rstd[e];                   // y exactly as the forward forms it
      shift[e] = beta[c + e] - st[e] * scale[e];
    }
  }
  // frame f of the clip at xs: xhat, and dy (zero where `read` is false: past the last frame layer 1 reads)
  __device__ __forceinline__ void frame(const float* __restrict__ xs, float* x, const unsigned short* __restrict__ dwin, int f, int c,
                                        int C0, int k0, int s0, int k1, int s1, int T1, bool read, float* xhat, float* dy) const {
#pragma unroll
    for (int j = 0; j < K0; ++j) x[j] = j < k0 ? xs[(size_t)f * s0 + j] : 0.0f;
    float v[8], da[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = 0.0f;
#pragma unroll
      for (int j = 0; j < K0; ++j) a = fmaf(cv.w[e][j], x[j], a);
      v[e] = a;
      xhat[e] = (a - mean[e]) * rstd[e];
      dy[e] = 0.0f;
    }
    if (read && w2v_fold8(dwin, f, c, C0, k1, s1, T1, da)) {
#pragma unroll
      for (int e = 0; e < 8; ++e) dy[e] = da[e] * gelu_erf_grad(fmaf(v[e], scale[e], shift[e]));
    }
  }
};

// pass 1a: S1 = sum dy, S2 = sum dy xhat over this thread's frames f = slot, slot + nslots, ... -> partial[clip][slot][S1 | S2][C0]
template <int K0>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_bwd_partial_kernel(const float* __restrict__ wave, const float* __restrict__ wt, const float* __restrict__ stats,
                                  const float* __restrict__ gamma, const float* __restrict__ beta, const unsigned short* __restrict__ dwin,
                                  float* __restrict__ partial, int L, int C0, int k0, int s0, int k1, int s1, int T1, float eps,
                                  int nfl, int cgn) {
  const int cgi = threadIdx.x % cgn, fl = threadIdx.x / cgn;
  if (fl >= nfl) return;
  const int slot = blockIdx.x * nfl + fl, nslots = gridDim.x * nfl, c = cgi * 8;
  Conv0Bwd<K0> b;
  b.load(wt, stats + (size_t)blockIdx.y * 2 * C0 + c, gamma, beta, c, C0, k0, eps);
  const float* __restrict__ xs = wave + (size_t)blockIdx.y * L;
  const unsigned short* __restrict__ g = dwin + (size_t)blockIdx.y * T1 * k1 * C0;
  const int last = s1 * (T1 - 1) + k1 - 1;                 // the last frame layer 1 reads: dy is zero past it
  float s1v[8], s2v[8], x[K0], xhat[8], dy[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s1v[e] = s2v[e] = 0.0f;
  for (int f = slot; f <= last; f += nslots) {
    b.frame(xs, x, g, f, c, C0, k0, s0, k1, s1, T1, true, xhat, dy);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s1v[e] += dy[e];
      s2v[e] = fmaf(dy[e], xhat[e], s2v[e]);
    }
  }
  float* __restrict__ p = partial + (((size_t)blockIdx.y * W2V_SLOTS + slot) * 2) * C0 + c;
  *reinterpret_cast<f32x4_t*>(p) = f32x4_t{s1v[0], s1v[1], s1v[2], s1v[3]};
  *reinterpret_cast<f32x4_t*>(p + 4) = f32x4_t{s1v[4], s1v[5], s1v[6], s1v[7]};
  *reinterpret_cast<f32x4_t*>(p + C0) = f32x4_t{s2v[0], s2v[1], s2v[2], s2v[3]};
  *reinterpret_cast<f32x4_t*>(p + C0 + 4) = f32x4_t{s2v[4], s2v[5], s2v[6], s2v[7]};
}

// pass 1b: the slots of one (clip, channel) added in slot order -> sums[clip][S1 | S2][C0]
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_bwd_merge_kernel(const float* __restrict__ partial, float* __restrict__ sums, int C0, int nslots) {
  const int c = blockIdx.x * W2V_THREADS + threadIdx.x;
  if (c >= C0) return;
  const float* __restrict__ p = partial + (size_t)blockIdx.y * W2V_SLOTS * 2 * C0 + c;
  float a = 0.0f, b = 0.0f;
  for (int s = 0; s < nslots; ++s) {
    a += p[(size_t)s * 2 * C0];
    b += p[(size_t)s * 2 * C0 + C0];
  }
  sums[(size_t)blockIdx.y * 2 * C0 + c] = a;
  sums[(size_t)blockIdx.y * 2 * C0 + C0 + c] = b;
}

// pass 1c: dbeta (+)= sum_n S1, dgamma (+)= sum_n S2, the clips in order
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_bwd_affine_kernel(const float* __restrict__ sums, float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int C0,
                                 int accumulate) {
  const int c = blockIdx.x * W2V_THREADS + threadIdx.x;
  if (c >= C0) return;
  float a = accumulate ? dbeta[c] : 0.0f, b = accumulate ? dgamma[c] : 0.0f;
  for (int n = 0; n < N; ++n) {
    a += sums[(size_t)n * 2 * C0 + c];
    b += sums[(size_t)n * 2 * C0 + C0 + c];
  }
  dbeta[c] = a;
  dgamma[c] = b;
}

// pass 2a: dc = gamma rstd (dy - S1 / T0 - xhat S2 / T0) on ALL T0 frames (a frame layer 1 never reads has dy = 0 but took part in
// the statistics), dW0[ch][j] partial = sum over this thread's frames of dc[ch] wave[s0 f + j] -> partial[clip * nslots + slot][C0][k0]
template <int K0>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_bwd_wgrad_kernel(const float* __restrict__ wave, const float* __restrict__ wt, const float* __restrict__ stats,
                                const float* __restrict__ gamma, const float* __restrict__ beta, const unsigned short* __restrict__ dwin,
                                const float* __restrict__ sums, float* __restrict__ partial, int L, int T0, int C0, int k0, int s0,
                                int k1, int s1, int T1, float eps, int nfl, int cgn) {
  const int cgi = threadIdx.x % cgn, fl = threadIdx.x / cgn;
  if (fl >= nfl) return;
  const int slot = blockIdx.x * nfl + fl, nslots = gridDim.x * nfl, c = cgi * 8;
  Conv0Bwd<K0> b;
  b.load(wt, stats + (size_t)blockIdx.y * 2 * C0 + c, gamma, beta, c, C0, k0, eps);
  const float* __restrict__ xs = wave + (size_t)blockIdx.y * L;
  const unsigned short* __restrict__ g = dwin + (size_t)blockIdx.y * T1 * k1 * C0;
  const float* __restrict__ sm = sums + (size_t)blockIdx.y * 2 * C0 + c;
  const int last = s1 * (T1 - 1) + k1 - 1;
  const float inv = 1.0f / (float)T0;
  float m1[8], m2[8], acc[8][K0], x[K0], xhat[8], dy[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m1[e] = sm[e] * inv;
    m2[e] = sm[C0 + e] * inv;
#pragma unroll
    for (int j = 0; j < K0; ++j) acc[e][j] = 0.0f;
  }
  for (int f = slot; f < T0; f += nslots) {
    b.frame(xs, x, g, f, c, C0, k0, s0, k1, s1, T1, f <= last, xhat, dy);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dc = b.scale[e] * (dy[e] - m1[e] - xhat[e] * m2[e]);
#pragma unroll
      for (int j = 0; j < K0; ++j) acc[e][j] = fmaf(dc, x[j], acc[e][j]);
    }
  }
  float* __restrict__ p = partial + ((size_t)blockIdx.y * nslots + slot) * C0 * k0 + (size_t)c * k0;
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int j = 0; j < K0; ++j)
      if (j < k0) p[e * k0 + j] = acc[e][j];
}

// pass 2b: dW0 (+)= the sum of the rows of partial (clip-major, then slot).  A workgroup owns WM_COLS output elements; its WM_RUNS
// thread rows each add one contiguous run of partial rows in order, and the runs' sums are added in run order: a fixed tree
constexpr int WM_COLS = 32, WM_RUNS = W2V_THREADS / WM_COLS;
__global__ __launch_bounds__(W2V_THREADS)
void w2v_conv0_bwd_wgrad_merge_kernel(const float* __restrict__ partial, float* __restrict__ dw, int numel, int rows, int accumulate) {
  __shared__ float part[WM_RUNS][WM_COLS];
  const int col = threadIdx.x % WM_COLS, run = threadIdx.x / WM_COLS, i = blockIdx.x * WM_COLS + col;
  const int per = (rows + WM_RUNS - 1) / WM_RUNS, r0 = run * per, r1 = min(rows, r0 + per);
  float a = 0.0f;
  if (i < numel)
    for (int r = r0; r < r1; ++r) a += partial[(size_t)r * numel + i];
  part[run][col] = a;
  __syncthreads();
  if (run == 0 && i < numel) {
    float s = accumulate ? dw[i] : 0.0f;
#pragma unroll
    for (int g = 0; g < WM_RUNS; ++g) s += part[g][col];
    dw[i] = s;
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
// The backward runs the same body twice more (EPI): with ``aux`` (N, T, C) bf16 the operand its epilogue reads at the output's place,
//   PC_FWD    y  = aux + gelu(acc + b)        aux = x: the forward
//   PC_ACT    dz = aux * gelu'(acc + b)       aux = dy: z = b + conv(x) is computed again, not stored
//   PC_DGRAD  dx = aux + acc                  aux = dy, x = dz, w = the weight with its taps reversed and co / ci swapped, and
//                                             pad = k - 1 - k/2 rows in front instead of k/2 (they differ for an even k)
enum { PC_FWD = 0, PC_ACT = 1, PC_DGRAD = 2 };
template <int CT, int EPI>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_posconv_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ wp, const float* __restrict__ bias,
                        const unsigned short* aux, unsigned short* y, int T, int C, int k, int Kp, int pad) {
  constexpr int CG = CT * 16, TT = 128;
  extern __shared__ __attribute__((aligned(16))) unsigned short sx[];
  const int t0 = blockIdx.x * TT, g = blockIdx.y;
  const unsigned short* __restrict__ xn = x + (size_t)blockIdx.z * T * C + g * CG;
  const unsigned short* an = aux + (size_t)blockIdx.z * T * C + g * CG;
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
      const u32x2_t xr = *reinterpret_cast<const u32x2_t*>(an + (size_t)t * C + co);
      u32x2_t o;
      if constexpr (EPI == PC_DGRAD) {
        const f32x4_t a = acc[tt][ct];
        o = u32x2_t{pack_bf16x2(bf16lo(xr[0]) + a[0], bf16hi(xr[0]) + a[1]), pack_bf16x2(bf16lo(xr[1]) + a[2], bf16hi(xr[1]) + a[3])};
      } else {
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(bias + g * CG + co);
        const f32x4_t a = acc[tt][ct] + b;
        if constexpr (EPI == PC_FWD)
          o = u32x2_t{pack_bf16x2(bf16lo(xr[0]) + gelu_erf(a[0]), bf16hi(xr[0]) + gelu_erf(a[1])),
                      pack_bf16x2(bf16lo(xr[1]) + gelu_erf(a[2]), bf16hi(xr[1]) + gelu_erf(a[3]))};
        else
          o = u32x2_t{pack_bf16x2(bf16lo(xr[0]) * gelu_erf_grad(a[0]), bf16hi(xr[0]) * gelu_erf_grad(a[1])),
                      pack_bf16x2(bf16lo(xr[1]) * gelu_erf_grad(a[2]), bf16hi(xr[1]) * gelu_erf_grad(a[3]))};
      }
      *reinterpret_cast<u32x2_t*>(y + ((size_t)blockIdx.z * T + t) * C + g * CG + co) = o;
    }
  }
}

// ---- positional convolution: weight gradient ----------------------------------------------------------------
// dW[g][co][j*CG + ci] (+)= sum_{n, t} dz[n][t][g*CG + co] * x[n][t + j - pad][g*CG + ci], rows outside [0, T) read as zero: per
// tap a (CG x CG) GEMM whose contraction runs over time.  One workgroup = (WG_TAPS = 8 taps, group, row slab); wave w owns taps
// 2w and 2w + 1 with all CT x CT output tiles in accumulators (2 * CT * CT * 4 f32 per lane) and the workgroup walks the slab's
// (clip, 128-row time block) units: the group's channels of the block's dz rows and of the x rows [t0 + j0 - pad, + 128 + 7) are
// staged as (rows, CG) images like the forward's, the next unit's rows are fetched into registers while this one is multiplied.
// Both operands of v_mfma_f32_16x16x32_bf16 have time as their 32-index and are read with ds_read_b64_tr_b16: A[row = co][k = time]
// from the dz image, B[k = time][col = ci] from the x image, where tap j is a row offset only (every row starts at a multiple of
// 32 bytes, CG being a multiple of 16).  The MFMA's k index 8 (lane >> 4) + e is time row 4 (lane >> 4) + e for e < 4 and
// 16 + 4 (lane >> 4) + e - 4 above, in both operands alike: the two 16-lane groups of a 32-lane half then read 8 CONSECUTIVE rows,
// which at CG = 48 (row stride 24 banks) are 8 different multiples of 8 banks, conflict-free; CG = 16 likewise, CG = 32 is 2-way
// and CG = 64 4-way conflicted (no shipped model has them).  EXEC is all ones at every transposed read: nothing around them
// branches on a lane, rows past T and taps past k are zeros / computed and dropped (pad, don't mask).
// D[row = co = 4 (lane >> 4) + reg][col = ci = lane & 15].  No atomics: with slabs > 1 slab s writes its own (C, Kp) partial.
constexpr int WG_TT = 128, WG_TAPS = 8;

template <int CT>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_posconv_wgrad_kernel(const unsigned short* __restrict__ dz, const unsigned short* __restrict__ x, float* __restrict__ dw,
                              int T, int C, int k, int Kp, int pad, int nblk, int units, int per_slab, int accumulate) {
  constexpr int CG = CT * 16, XR = WG_TT + WG_TAPS - 1;
  constexpr int NZ = WG_TT * CG / 8, NX = XR * CG / 8, NV = (NZ + NX + W2V_THREADS - 1) / W2V_THREADS;
  __shared__ __attribute__((aligned(16))) unsigned short sz[WG_TT * CG];
  __shared__ __attribute__((aligned(16))) unsigned short sxr[XR * CG];
  const int j0 = blockIdx.x * WG_TAPS, g = blockIdx.y;
  const int u0 = blockIdx.z * per_slab, u1 = min(units, u0 + per_slab);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  float* __restrict__ out = dw + (size_t)blockIdx.z * C * Kp;                        // slab s writes partial s
  u32x4_t pre[NV];
  auto fetch = [&](int u) {
    const int n = u / nblk, t0 = (u - n * nblk) * WG_TT;
    const unsigned short* __restrict__ zn = dz + (size_t)n * T * C + g * CG;
    const unsigned short* __restrict__ xn = x + (size_t)n * T * C + g * CG;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * W2V_THREADS;
      u32x4_t val = {0u, 0u, 0u, 0u};
      if (v < NZ) {
        const int e = v << 3, rr = e / CG, cc = e - rr * CG, t = t0 + rr;
        if (t < T) val = *reinterpret_cast<const u32x4_t*>(zn + (size_t)t * C + cc);
      } else if (v < NZ + NX) {
        const int e = (v - NZ) << 3, rr = e / CG, cc = e - rr * CG, t = t0 + j0 - pad + rr;
        if (t >= 0 && t < T) val = *reinterpret_cast<const u32x4_t*>(xn + (size_t)t * C + cc);
      }
      pre[i] = val;
    }
  };
  f32x4_t acc[2][CT][CT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < CT; ++b)
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[a][b][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  auto tr8 = [](const unsigned short* at) {                            // rows r .. r + 3 and r + 16 .. r + 19 of 16 columns
    const s16x4_t lo = lds_read_tr16(at), hi = lds_read_tr16(at + 16 * CG);
    const s16x8_t w = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, w);
  };
  if (u0 < u1) fetch(u0);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();                                                   // the previous unit's reads are done
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * W2V_THREADS;
      if (v < NZ) *reinterpret_cast<u32x4_t*>(sz + (v << 3)) = pre[i];
      else if (v < NZ + NX) *reinterpret_cast<u32x4_t*>(sxr + ((v - NZ) << 3)) = pre[i];
    }
    __syncthreads();
    if (u + 1 < u1) fetch(u + 1);
#pragma unroll
    for (int ks = 0; ks < WG_TT / 32; ++ks) {
      const int row = ks * 32 + 4 * gq + q;
      bf16x8_t az[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) az[ct] = tr8(sz + row * CG + ct * 16 + 4 * p);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ci = 0; ci < CT; ++ci) {
          const bf16x8_t b = tr8(sxr + (row + 2 * wave + a) * CG + ci * 16 + 4 * p);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) acc[a][ct][ci] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az[ct], b, acc[a][ct][ci], 0, 0, 0);
        }
    }
  }
  const int r = lane & 15;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int j = j0 + 2 * wave + a;
    if (j > k) continue;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int ci = 0; ci < CT; ++ci)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = j * CG + ci * 16 + r;
          if (col >= Kp) continue;                                     // tap k is the zero padding of the rows, where Kp has any
          float* dst = out + (size_t)(g * CG + ct * 16 + 4 * gq + e) * Kp + col;
          const float val = j < k ? acc[a][ct][ci][e] : 0.0f;
          *dst = accumulate ? *dst + val : val;
        }
  }
}

// ---- weight norm: dW_eff -> dg, dv ------------------------------------------------------------------------------
// w_eff[c][ci][j] = g[j] u, u = v[c][ci][j] / ||v[:, :, j]||: dg[j] = sum dW u, dv = (g / ||v||) (dW - u dg[j]).  One workgroup per tap j;
// dw is the packed (C, Kp) gradient (column j*cg + ci), v / dv (C, cg, k) f32.  f32 throughout; a lane sums its elements in index
// order, the wave sums by xor-shuffles and the four waves' sums are added in wave order: the same bits on every run.
__global__ __launch_bounds__(W2V_THREADS)
void w2v_weightnorm_bwd_kernel(const float* __restrict__ dw, const float* __restrict__ gain, const float* __restrict__ v,
                               float* __restrict__ dg, float* __restrict__ dv, int n /* C*cg */, int cg, int k, int Kp, int overwrite_v) {
  __shared__ float red[2][W2V_THREADS / 64];
  const int j = blockIdx.x;
  float svv = 0.0f, sdv = 0.0f;
  for (int e = threadIdx.x; e < n; e += W2V_THREADS) {
    const int c = e / cg, ci = e - c * cg;
    const float vv = v[(size_t)e * k + j], d = dw[(size_t)c * Kp + j * cg + ci];
    svv = fmaf(vv, vv, svv);
    sdv = fmaf(d, vv, sdv);
  }
  svv = wave_sum(svv);
  sdv = wave_sum(sdv);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = svv; red[1][threadIdx.x >> 6] = sdv; }
  __syncthreads();
  svv = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  sdv = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  const float inv = rsqrtf(svv), dgj = sdv * inv, scale = gain[j] * inv;
  if (threadIdx.x == 0) dg[j] += dgj;
  for (int e = threadIdx.x; e < n; e += W2V_THREADS) {
    const int c = e / cg, ci = e - c * cg;
    const size_t at = (size_t)e * k + j;
    const float val = scale * (dw[(size_t)c * Kp + j * cg + ci] - v[at] * inv * dgj);
    dv[at] = overwrite_v ? val : dv[at] + val;
  }
}

// ---- training-mode regularisers: the time-mask draw, mask + feature-projection dropout -------------------------------------
// The span count of HuggingFace's _compute_mask_indices for a drawn count `num` (no attention mask): raised to min_masks, T / length
// where the spans would be longer than the clip, at most T - (length - 1).  Host and device; monotone in num.
__host__ __device__ inline int w2v_span_count(long long num, int T, int length, int min_masks) {
  if (num < min_masks) num = min_masks;
  if (num * length > T) num = T / length;
  const int room = T - (length - 1);
  if (num > room) num = room > 0 ? room : 0;
  return (int)num;
}

// One lane per clip: starts[clip][0 .. S_max) = the clip's span starts, -1 in the unused slots.  Draw n of clip c is
// mmf_mix32(key + n * 0x9E3779B9) with key = mmf_rng_key(state, site, item0 + c) (mmf_keep's hash before its threshold):
//   draw 0         the count: n0 + (draw >= up), the integer form of int(prob T / length + u), u = draw / 2^32 (the host forms
//                  n0 = floor(e) and up = ceil((1 - frac(e)) 2^32) from e = prob T / length in double), then w2v_span_count
//   draws 1, 2, .. the starts, uniform in 0 .. T - length as (draw * (T - length + 1)) >> 32; a start already taken is drawn again,
//                  MASK_TRIES draws at most per start; after that the start is the next free value above the last draw, cyclically
//                  (there is one: the count is at most T - length + 1).  Spans may overlap, as in HuggingFace.
constexpr int MASK_TRIES = 64;
__global__ __launch_bounds__(64)
void w2v_mask_spans_kernel(int* __restrict__ starts, int N, int S_max, int T, int length, int n0, unsigned long long up, int min_masks,
                           const unsigned long long* __restrict__ state, unsigned site, unsigned item0) {
  const int clip = blockIdx.x * 64 + threadIdx.x;
  if (clip >= N) return;
  const unsigned key = mmf_rng_key(*state, site, item0 + (unsigned)clip);
  unsigned n = 0u;
  auto draw = [&]() { return mmf_mix32(key + (n++) * 0x9E3779B9u); };
  const unsigned range = (unsigned)(T - length + 1);
  int num = w2v_span_count((long long)n0 + ((unsigned long long)draw() >= up ? 1 : 0), T, length, min_masks);
  num = num < S_max ? num : S_max;
  int* row = starts + (size_t)clip * S_max;
  auto taken = [&](int cand, int k) {
    for (int i = 0; i < k; ++i)
      if (row[i] == cand) return true;
    return false;
  };
  for (int k = 0; k < num; ++k) {
    int cand = 0;
    bool free_ = false;
    for (int a = 0; a < MASK_TRIES && !free_; ++a) {
      cand = (int)(((unsigned long long)draw() * range) >> 32);
      free_ = !taken(cand, k);
    }
    for (unsigned a = 0; a < range && !free_; ++a) {
      cand = cand + 1 == (int)range ? 0 : cand + 1;
      free_ = !taken(cand, k);
    }
    row[k] = cand;
  }
  for (int k = num; k < S_max; ++k) row[k] = -1;
}

__device__ __forceinline__ bool w2v_in_span(const int* __restrict__ row, int S_max, int length, int t) {
  bool in = false;
  for (int k = 0; k < S_max; ++k) {
    const int s = row[k];
    in |= s >= 0 && (unsigned)(t - s) < (unsigned)length;
  }
  return in;
}

// out = a row inside a span ? (EMBED: bf16(embed), else 0) : keep ? x c : 0, one pass over `items` clips of (T, d) bf16, eight elements per
// lane; out may be x.  starts: the clips' rows of the span table or NULL (no masking); a threshold of 0 keeps everything (c = 1).  The mask of
// element (t, j) of clip g is drawn from sub-stream item0 + g at index t d + j.  blockIdx.y walks the clips.
template <bool EMBED>
__global__ __launch_bounds__(W2V_THREADS)
void w2v_mask_drop_kernel(const unsigned short* x, const float* __restrict__ embed, const int* __restrict__ starts, unsigned short* out,
                          unsigned items, unsigned T, unsigned d8 /* d / 8 */, int S_max, int length, const MmfItemDrop dr) {
  const unsigned long long state = dr.thresh ? *dr.state : 0ull;
  const unsigned per8 = T * d8;
  for (unsigned g = blockIdx.y; g < items; g += gridDim.y) {
    const unsigned key = mmf_rng_key(state, dr.site, dr.item0 + g);
    const int* row = starts ? starts + (size_t)g * S_max : nullptr;
    for (unsigned v = blockIdx.x * W2V_THREADS + threadIdx.x; v < per8; v += gridDim.x * W2V_THREADS) {
      const unsigned t = v / d8, j = (v - t * d8) << 3;
      const size_t at = ((size_t)g * per8 + v) * 8;
      float f[8];
      if (row && w2v_in_span(row, S_max, length, (int)t)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = EMBED ? embed[j + e] : 0.0f;
      } else {
        unpack8(*reinterpret_cast<const u32x4_t*>(x + at), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = mmf_keep(key, v * 8u + (unsigned)e, dr.thresh) ? f[e] * dr.inv_keep : 0.0f;
      }
      *reinterpret_cast<u32x4_t*>(out + at) = pack8(f);
    }
  }
}

// partial[slab][col] = the sum over the slab's rows that lie inside a span of dx[row][col], f32, rows in order: one lane per column,
// blockIdx.y the slab of `per` rows.  mmf_sum_slabs_f32 adds the slabs in order, so the embedding's gradient has the same bits on every run.
__global__ __launch_bounds__(W2V_THREADS)
void w2v_mask_embed_grad_kernel(const unsigned short* __restrict__ dx, const int* __restrict__ starts, float* __restrict__ partial, int rows,
                                int T, int d, int S_max, int length, int per) {
  const int col = blockIdx.x * W2V_THREADS + threadIdx.x, r0 = blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
  if (col >= d) return;
  float acc = 0.0f;
  for (int r = r0; r < r1; ++r) {
    const int g = r / T, t = r - g * T;
    if (w2v_in_span(starts + (size_t)g * S_max, S_max, length, t)) acc += bf16_bits_to_f32(dx[(size_t)r * d + col]);
  }
  partial[(size_t)blockIdx.y * d + col] = acc;
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

namespace {
// the channel counts the layer-norm kernels reduce over: C / 8 lanes, a power of two up to 256 (8 .. 2048 channels)
bool w2v_ln_channels(int C) { return C >= 8 && C <= 2048 && (C & 7) == 0 && ((C >> 3) & ((C >> 3) - 1)) == 0; }
}  // namespace

extern "C" int mmf_w2v_conv0_ln_gelu(const float* wave, const float* weight, const float* bias, const float* gamma, const float* beta,
                                     void* out_bf16, int N, int L, int C0, int k0, int s0, int k1, int s1, float eps, void* stream) {
  const char* fn = "mmf_w2v_conv0_ln_gelu";
  if (!wave || !weight || !gamma || !beta || !out_bf16) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", fn);
  Conv0Shape sh;
  if (int rc = conv0_check(fn, N, L, C0, k0, s0, &sh)) return rc;
  if (!w2v_ln_channels(C0)) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: C0=%d: C0 / 8 must be a power of two up to 256", fn, C0);
  if (k1 <= 0 || s1 <= 0 || sh.T0 < k1) MMF_FAIL(MMF_E_SHAPE, "%s: k1=%d s1=%d against T0=%d frames", fn, k1, s1, sh.T0);
  const int T1 = (sh.T0 - k1) / s1 + 1;
  if (k1 < s1 || (int64_t)T1 * k1 * (C0 / 8) >= (int64_t)1 << 31)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: k1=%d >= s1=%d, %lld window elements per clip (below 2^34)", fn, k1, s1, (long long)T1 * k1 * C0);
  if (!mmf_aligned16(out_bf16) || (reinterpret_cast<uintptr_t>(wave) & 3u) || (reinterpret_cast<uintptr_t>(weight) & 3u)
      || (reinterpret_cast<uintptr_t>(bias) & 3u) || (reinterpret_cast<uintptr_t>(gamma) & 3u) || (reinterpret_cast<uintptr_t>(beta) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "%s: out must be 16-byte aligned, the f32 operands 4-byte aligned", fn);
  const int cgn = C0 / 8, nfl = W2V_THREADS / cgn;
  int64_t blocks = ((int64_t)s1 * (T1 - 1) + k1 + nfl - 1) / nfl;
  if (blocks > 1024) blocks = 1024;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned short* out = static_cast<unsigned short*>(out_bf16);
  if (k0 <= 10) hipLaunchKernelGGL(w2v_conv0_ln_gelu_kernel<10>, dim3((int)blocks, N), dim3(W2V_THREADS), 0, s, wave, weight, bias, gamma, beta, out, L, C0, k0, s0, k1, s1, T1, eps, nfl, cgn);
  else          hipLaunchKernelGGL(w2v_conv0_ln_gelu_kernel<16>, dim3((int)blocks, N), dim3(W2V_THREADS), 0, s, wave, weight, bias, gamma, beta, out, L, C0, k0, s0, k1, s1, T1, eps, nfl, cgn);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_w2v_ln_gelu_window(const void* x_bf16, const float* gamma, const float* beta, void* out_bf16, int N, int T_in, int C,
                                      int k, int s, float eps, void* stream) {
  const char* fn = "mmf_w2v_ln_gelu_window";
  if (!x_bf16 || !gamma || !beta || !out_bf16 || N <= 0 || T_in <= 0 || C <= 0 || k < 0 || (k > 0 && s <= 0))
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or N=%d T_in=%d C=%d k=%d s=%d", fn, N, T_in, C, k, s);
  if (T_in < k) MMF_FAIL(MMF_E_SHAPE, "%s: T_in=%d is shorter than the kernel k=%d", fn, T_in, k);
  if (!w2v_ln_channels(C)) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: C=%d: C / 8 must be a power of two up to 256", fn, C);
  const int64_t T_out = k ? (T_in - k) / s + 1 : T_in, T_read = k ? (int64_t)s * (T_out - 1) + k : T_in;
  const int64_t nvec = T_out * (k ? k : 1) * (C / 8);
  if ((k > 0 && k < s) || N > 65535 || nvec >= (int64_t)1 << 31 || (k > 0 && x_bf16 == out_bf16))
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: k=%d >= s=%d (or k = 0), N=%d (at most 65535), %lld output elements per clip (below 2^34), out may "
             "be x for k = 0 only", fn, k, s, N, (long long)nvec * 8);
  if (!mmf_aligned16(x_bf16) || !mmf_aligned16(out_bf16) || (reinterpret_cast<uintptr_t>(gamma) & 3u) || (reinterpret_cast<uintptr_t>(beta) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "%s: x / out must be 16-byte aligned, gamma / beta 4-byte aligned", fn);
  const int cgn = C / 8, rpb = W2V_THREADS / cgn;
  // up to 8 passes per workgroup where that still leaves 2048 workgroups: a lane's gamma / beta (64 bytes) are then loaded once for
  // 8 rows' 16 bytes each
  const int64_t row_blocks = (T_read + rpb - 1) / rpb;
  int64_t passes = (int64_t)N * row_blocks / 2048;
  if (passes > 8) passes = 8;
  if (passes < 1) passes = 1;
  hipLaunchKernelGGL(w2v_ln_gelu_window_kernel, dim3(mmf_stream_grid((row_blocks + passes - 1) / passes, 1), N), dim3(W2V_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned short*>(x_bf16), gamma, beta, static_cast<unsigned short*>(out_bf16),
                     T_in, (int)T_read, (int)T_out, C, k, s, eps, rpb, cgn);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_w2v_window_fold_gelu_bwd(const void* dwin_bf16, const void* x_bf16, void* dx_bf16, int N, int T_in, int C, int k, int s,
                                            void* stream) {
  if (!dwin_bf16 || !x_bf16 || !dx_bf16 || N <= 0 || T_in <= 0 || C <= 0 || k <= 0 || s <= 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_window_fold_gelu_bwd: null operand or N=%d T_in=%d C=%d k=%d s=%d", N, T_in, C, k, s);
  if (T_in < k) MMF_FAIL(MMF_E_SHAPE, "mmf_w2v_window_fold_gelu_bwd: T_in=%d is shorter than the kernel k=%d", T_in, k);
  const int64_t T_out = (T_in - k) / s + 1, wvec = T_out * k * (C / 8), nvec = (int64_t)T_in * (C / 8);
  if ((C & 7) || k < s || N > 65535 || wvec >= (int64_t)1 << 31 || nvec >= (int64_t)1 << 31 || dwin_bf16 == x_bf16 || dwin_bf16 == dx_bf16)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_w2v_window_fold_gelu_bwd: C=%d (multiple of 8), k=%d >= s=%d, N=%d (at most 65535), %lld window "
             "elements per clip (below 2^34), dwin must be neither x nor dx", C, k, s, N, (long long)wvec * 8);
  if (!mmf_aligned16(dwin_bf16) || !mmf_aligned16(x_bf16) || !mmf_aligned16(dx_bf16))
    MMF_FAIL(MMF_E_ALIGN, "mmf_w2v_window_fold_gelu_bwd: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(w2v_window_fold_gelu_bwd_kernel, dim3(mmf_stream_grid(nvec, W2V_THREADS), N), dim3(W2V_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned short*>(dwin_bf16), static_cast<const unsigned short*>(x_bf16),
                     static_cast<unsigned short*>(dx_bf16), T_in, (int)T_out, C, k, s, (unsigned)(C / 8), (unsigned)nvec);
  MMF_CHECK_LAUNCH("mmf_w2v_window_fold_gelu_bwd");
  return MMF_OK;
}

namespace {

// shared validation of layer 0's two backward entry points -> the launch shape of mmf_w2v_conv0_stats (nblk workgroups of nfl frame lanes)
int conv0_bwd_check(const char* fn, const void* const* f32s, int nf32, const void* dwin, int N, int L, int C0, int k0, int s0, int k1,
                    int s1, Conv0Shape* sh, int* nblk) {
  for (int i = 0; i < nf32; ++i)
    if (!f32s[i]) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", fn);
  if (!dwin) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", fn);
  if (int rc = conv0_check(fn, N, L, C0, k0, s0, sh)) return rc;
  if (k1 <= 0 || s1 <= 0 || sh->T0 < k1) MMF_FAIL(MMF_E_SHAPE, "%s: k1=%d s1=%d against T0=%d frames", fn, k1, s1, sh->T0);
  sh->T1 = (sh->T0 - k1) / s1 + 1;
  if ((int64_t)sh->T1 * k1 * (C0 / 8) >= (int64_t)1 << 31)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: %lld window elements per clip (below 2^34)", fn, (long long)sh->T1 * k1 * C0);
  if (!mmf_aligned16(dwin)) MMF_FAIL(MMF_E_ALIGN, "%s: dwin_1 must be 16-byte aligned", fn);
  for (int i = 0; i < nf32; ++i)
    if (reinterpret_cast<uintptr_t>(f32s[i]) & 3u) MMF_FAIL(MMF_E_ALIGN, "%s: the f32 operands must be 4-byte aligned", fn);
  *nblk = sh->nblk;
  if ((int64_t)*nblk * sh->nfl > sh->T0) *nblk = (sh->T0 + sh->nfl - 1) / sh->nfl;
  return MMF_OK;
}

}  // namespace

extern "C" int mmf_w2v_conv0_bwd_stats(const float* wave, const float* weight, const float* stats, const float* gamma, const float* beta,
                                       const void* dwin1_bf16, float* sums, float* partial, float* dgamma, float* dbeta, int N, int L,
                                       int C0, int k0, int s0, int k1, int s1, float eps, int accumulate, void* stream) {
  const char* fn = "mmf_w2v_conv0_bwd_stats";
  const void* f32s[] = {wave, weight, stats, gamma, beta, sums, partial, dgamma, dbeta};
  Conv0Shape sh;
  int nblk;
  if (int rc = conv0_bwd_check(fn, f32s, 9, dwin1_bf16, N, L, C0, k0, s0, k1, s1, &sh, &nblk)) return rc;
  if (!mmf_aligned16(stats) || !mmf_aligned16(sums) || !mmf_aligned16(partial))
    MMF_FAIL(MMF_E_ALIGN, "%s: stats / sums / partial must be 16-byte aligned", fn);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned short* dwin = static_cast<const unsigned short*>(dwin1_bf16);
  const int nslots = nblk * sh.nfl;                                       // <= MMF_W2V_STATS_SLOTS
  if (k0 <= 10) hipLaunchKernelGGL(w2v_conv0_bwd_partial_kernel<10>, dim3(nblk, N), dim3(W2V_THREADS), 0, s, wave, weight, stats, gamma, beta, dwin, partial, L, C0, k0, s0, k1, s1, sh.T1, eps, sh.nfl, sh.cgn);
  else          hipLaunchKernelGGL(w2v_conv0_bwd_partial_kernel<16>, dim3(nblk, N), dim3(W2V_THREADS), 0, s, wave, weight, stats, gamma, beta, dwin, partial, L, C0, k0, s0, k1, s1, sh.T1, eps, sh.nfl, sh.cgn);
  MMF_CHECK_LAUNCH(fn);
  const int cblk = (C0 + W2V_THREADS - 1) / W2V_THREADS;
  hipLaunchKernelGGL(w2v_conv0_bwd_merge_kernel, dim3(cblk, N), dim3(W2V_THREADS), 0, s, partial, sums, C0, nslots);
  MMF_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(w2v_conv0_bwd_affine_kernel, dim3(cblk), dim3(W2V_THREADS), 0, s, sums, dgamma, dbeta, N, C0, accumulate);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_w2v_conv0_bwd_wgrad(const float* wave, const float* weight, const float* stats, const float* gamma, const float* beta,
                                       const void* dwin1_bf16, const float* sums, float* partial, float* dweight, int N, int L, int C0,
                                       int k0, int s0, int k1, int s1, float eps, int accumulate, void* stream) {
  const char* fn = "mmf_w2v_conv0_bwd_wgrad";
  const void* f32s[] = {wave, weight, stats, gamma, beta, sums, partial, dweight};
  Conv0Shape sh;
  int nblk;
  if (int rc = conv0_bwd_check(fn, f32s, 8, dwin1_bf16, N, L, C0, k0, s0, k1, s1, &sh, &nblk)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned short* dwin = static_cast<const unsigned short*>(dwin1_bf16);
  const int nslots = nblk * sh.nfl;
  if (k0 <= 10) hipLaunchKernelGGL(w2v_conv0_bwd_wgrad_kernel<10>, dim3(nblk, N), dim3(W2V_THREADS), 0, s, wave, weight, stats, gamma, beta, dwin, sums, partial, L, sh.T0, C0, k0, s0, k1, s1, sh.T1, eps, sh.nfl, sh.cgn);
  else          hipLaunchKernelGGL(w2v_conv0_bwd_wgrad_kernel<16>, dim3(nblk, N), dim3(W2V_THREADS), 0, s, wave, weight, stats, gamma, beta, dwin, sums, partial, L, sh.T0, C0, k0, s0, k1, s1, sh.T1, eps, sh.nfl, sh.cgn);
  MMF_CHECK_LAUNCH(fn);
  const int numel = C0 * k0;
  hipLaunchKernelGGL(w2v_conv0_bwd_wgrad_merge_kernel, dim3((numel + WM_COLS - 1) / WM_COLS), dim3(W2V_THREADS), 0, s, partial, dweight, numel, N * nslots, accumulate);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

namespace {

// the three entry points of w2v_posconv_kernel: validation (``aux`` is x for the forward) and the launch of the EPI instantiation
template <int EPI>
int posconv_run(const char* fn, const void* x_bf16, const void* w_bf16, const float* bias, const void* aux_bf16, void* y_bf16, int N, int T,
                int C, int groups, int k, int pad, void* stream) {
  if (!x_bf16 || !w_bf16 || (EPI != PC_DGRAD && !bias) || !aux_bf16 || !y_bf16 || N <= 0 || T <= 0 || C <= 0 || groups <= 0 || k <= 0)
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or N=%d T=%d C=%d groups=%d k=%d", fn, N, T, C, groups, k);
  if (C % groups) MMF_FAIL(MMF_E_SHAPE, "%s: C=%d is not a multiple of groups=%d", fn, C, groups);
  const int cg = C / groups;
  if ((cg & 15) || cg > 64 || N > 65535 || groups > 65535 || x_bf16 == y_bf16)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: group width %d (16, 32, 48 or 64), N=%d groups=%d (at most 65535), %s", fn, cg, N, groups,
             EPI == PC_FWD ? "y must not be x" : "the output must not be the convolution's input");
  const int Kp = (k * cg + 31) & ~31;
  const size_t lds = ((size_t)127 * cg + Kp) * 2;
  if (lds > 65536) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: k=%d at group width %d needs %zu bytes of LDS (at most 65536)", fn, k, cg, lds);
  if (!mmf_aligned16(x_bf16) || !mmf_aligned16(w_bf16) || !mmf_aligned16(bias) || !mmf_aligned16(aux_bf16) || !mmf_aligned16(y_bf16))
    MMF_FAIL(MMF_E_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  const dim3 grid((T + 127) / 128, groups, N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned short* x = static_cast<const unsigned short*>(x_bf16);
  const unsigned short* w = static_cast<const unsigned short*>(w_bf16);
  const unsigned short* aux = static_cast<const unsigned short*>(aux_bf16);
  unsigned short* y = static_cast<unsigned short*>(y_bf16);
  switch (cg / 16) {
    case 1: hipLaunchKernelGGL((w2v_posconv_kernel<1, EPI>), grid, dim3(W2V_THREADS), lds, s, x, w, bias, aux, y, T, C, k, Kp, pad); break;
    case 2: hipLaunchKernelGGL((w2v_posconv_kernel<2, EPI>), grid, dim3(W2V_THREADS), lds, s, x, w, bias, aux, y, T, C, k, Kp, pad); break;
    case 3: hipLaunchKernelGGL((w2v_posconv_kernel<3, EPI>), grid, dim3(W2V_THREADS), lds, s, x, w, bias, aux, y, T, C, k, Kp, pad); break;
    default: hipLaunchKernelGGL((w2v_posconv_kernel<4, EPI>), grid, dim3(W2V_THREADS), lds, s, x, w, bias, aux, y, T, C, k, Kp, pad); break;
  }
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

}  // namespace

extern "C" int mmf_w2v_posconv(const void* x_bf16, const void* w_bf16, const float* bias, void* y_bf16, int N, int T, int C,
                               int groups, int k, void* stream) {
  return posconv_run<PC_FWD>("mmf_w2v_posconv", x_bf16, w_bf16, bias, x_bf16, y_bf16, N, T, C, groups, k, k >> 1, stream);
}

extern "C" int mmf_w2v_posconv_bwd_act(const void* x_bf16, const void* w_bf16, const float* bias, const void* dy_bf16, void* dz_bf16,
                                       int N, int T, int C, int groups, int k, void* stream) {
  return posconv_run<PC_ACT>("mmf_w2v_posconv_bwd_act", x_bf16, w_bf16, bias, dy_bf16, dz_bf16, N, T, C, groups, k, k >> 1, stream);
}

extern "C" int mmf_w2v_posconv_dgrad(const void* dz_bf16, const void* wt_bf16, const void* dy_bf16, void* dx_bf16, int N, int T, int C,
                                     int groups, int k, void* stream) {
  return posconv_run<PC_DGRAD>("mmf_w2v_posconv_dgrad", dz_bf16, wt_bf16, nullptr, dy_bf16, dx_bf16, N, T, C, groups, k, k - 1 - (k >> 1),
                               stream);
}

extern "C" int mmf_w2v_posconv_wgrad(const void* dz_bf16, const void* x_bf16, float* dw, int N, int T, int C, int groups, int k,
                                     int slabs, int accumulate, void* stream) {
  const char* fn = "mmf_w2v_posconv_wgrad";
  if (!dz_bf16 || !x_bf16 || !dw || N <= 0 || T <= 0 || C <= 0 || groups <= 0 || k <= 0 || slabs <= 0)
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or N=%d T=%d C=%d groups=%d k=%d slabs=%d", fn, N, T, C, groups, k, slabs);
  if (C % groups) MMF_FAIL(MMF_E_SHAPE, "%s: C=%d is not a multiple of groups=%d", fn, C, groups);
  const int cg = C / groups, nblk = (T + WG_TT - 1) / WG_TT;
  const int64_t units = (int64_t)N * nblk;
  if (slabs > units || slabs > MMF_SUM_SLABS_MAX || (slabs > 1 && accumulate))
    MMF_FAIL(MMF_E_SHAPE, "%s: slabs=%d must be at most %d and the %lld (clip, 128-row block) units, and slab partials are written, "
             "not added to (accumulate=%d)", fn, slabs, MMF_SUM_SLABS_MAX, (long long)units, accumulate);
  if ((cg & 15) || cg > 64 || N > 65535 || groups > 65535 || units >= ((int64_t)1 << 30))
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: group width %d (16, 32, 48 or 64), N=%d groups=%d (at most 65535)", fn, cg, N, groups);
  const int Kp = (k * cg + 31) & ~31;
  if (((size_t)127 * cg + Kp) * 2 > 65536)                             // the forward's limit: what it cannot run has no gradient to take
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: k=%d at group width %d is beyond the forward's LDS limit", fn, k, cg);
  if (!mmf_aligned16(dz_bf16) || !mmf_aligned16(x_bf16) || !mmf_aligned16(dw))
    MMF_FAIL(MMF_E_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned short* dz = static_cast<const unsigned short*>(dz_bf16);
  const unsigned short* x = static_cast<const unsigned short*>(x_bf16);
  const int per = (int)((units + slabs - 1) / slabs), pad = k >> 1;
  const dim3 grid((k + WG_TAPS - 1) / WG_TAPS, groups, slabs);
  const int nu = (int)units;
  switch (cg / 16) {
    case 1: hipLaunchKernelGGL(w2v_posconv_wgrad_kernel<1>, grid, dim3(W2V_THREADS), 0, s, dz, x, dw, T, C, k, Kp, pad, nblk, nu, per, accumulate); break;
    case 2: hipLaunchKernelGGL(w2v_posconv_wgrad_kernel<2>, grid, dim3(W2V_THREADS), 0, s, dz, x, dw, T, C, k, Kp, pad, nblk, nu, per, accumulate); break;
    case 3: hipLaunchKernelGGL(w2v_posconv_wgrad_kernel<3>, grid, dim3(W2V_THREADS), 0, s, dz, x, dw, T, C, k, Kp, pad, nblk, nu, per, accumulate); break;
    default: hipLaunchKernelGGL(w2v_posconv_wgrad_kernel<4>, grid, dim3(W2V_THREADS), 0, s, dz, x, dw, T, C, k, Kp, pad, nblk, nu, per, accumulate); break;
  }
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_w2v_weightnorm_bwd(const float* dw, const float* g, const float* v, float* dg, float* dv, int C, int cg, int k,
                                      int overwrite_v, void* stream) {
  const char* fn = "mmf_w2v_weightnorm_bwd";
  if (!dw || !g || !v || !dg || !dv || C <= 0 || cg <= 0 || k <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: null operand or C=%d cg=%d k=%d", fn, C, cg, k);
  if (C % cg) MMF_FAIL(MMF_E_SHAPE, "%s: C=%d is not a multiple of the group width %d", fn, C, cg);
  if (k > 65535 || (int64_t)C * cg >= ((int64_t)1 << 31) / k)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: k=%d (at most 65535), C * cg * k = %lld (below 2^31)", fn, k, (long long)C * cg * k);
  if (!mmf_aligned16(dw) || (reinterpret_cast<uintptr_t>(g) & 3u) || (reinterpret_cast<uintptr_t>(v) & 3u) || (reinterpret_cast<uintptr_t>(dg) & 3u)
      || (reinterpret_cast<uintptr_t>(dv) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "%s: dw must be 16-byte aligned, the other operands 4-byte aligned", fn);
  const int Kp = (k * cg + 31) & ~31;
  hipLaunchKernelGGL(w2v_weightnorm_bwd_kernel, dim3(k), dim3(W2V_THREADS), 0, static_cast<hipStream_t>(stream), dw, g, v, dg, dv, C * cg, cg, k, Kp,
                     overwrite_v);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

namespace {
int mask_geometry(const char* fn, int64_t items, int T, int S_max, int length) {
  if (items <= 0 || T <= 0 || S_max <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: items=%lld T=%d S_max=%d", fn, (long long)items, T, S_max);
  if (length < 1 || length > T) MMF_FAIL(MMF_E_SHAPE, "%s: length=%d must be in 1 .. T=%d", fn, length, T);
  if (items > ((int64_t)1 << 31) - 1 || items * (int64_t)S_max >= ((int64_t)1 << 31))
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: items=%lld x S_max=%d (below 2^31)", fn, (long long)items, S_max);
  return MMF_OK;
}
}  // namespace

extern "C" int mmf_w2v_mask_spans(int* starts, int N, int S_max, int T, double mask_prob, int length, int min_masks,
                                  const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream) {
  const char* fn = "mmf_w2v_mask_spans";
  if (!starts || !rng_state) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", fn);
  if (int rc = mask_geometry(fn, N, T, S_max, length)) return rc;
  if (!(mask_prob > 0.0) || mask_prob > 1.0 || min_masks < 0 || item0 < 0)
    MMF_FAIL(MMF_E_SHAPE, "%s: mask_prob=%g (in (0, 1]), min_masks=%d, item0=%lld", fn, mask_prob, min_masks, (long long)item0);
  if ((reinterpret_cast<uintptr_t>(starts) & 3u) || (reinterpret_cast<uintptr_t>(rng_state) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "%s: starts must be 4-byte aligned, rng_state 8-byte aligned", fn);
  const double e = mask_prob * (double)T / (double)length;
  const long long n0 = (long long)e;                                  // e >= 0: the floor
  const double up = (1.0 - (e - (double)n0)) * 4294967296.0;
  unsigned long long upi = (unsigned long long)up;
  if ((double)upi < up) ++upi;                                        // the ceiling: 2^32 (never) where e is whole
  if (w2v_span_count(n0 + 1, T, length, min_masks) > S_max)
    MMF_FAIL(MMF_E_SHAPE, "%s: S_max=%d is below the %d spans a clip may draw", fn, S_max, w2v_span_count(n0 + 1, T, length, min_masks));
  hipLaunchKernelGGL(w2v_mask_spans_kernel, dim3((N + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), starts, N, S_max, T, length,
                     (int)(n0 > T ? T : n0), upi, min_masks, reinterpret_cast<const unsigned long long*>(rng_state), site, (unsigned)item0);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_w2v_mask_drop(const void* x_bf16, const float* embed, const int* starts, void* out_bf16, int64_t items, int T, int d,
                                 int S_max, int length, float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream) {
  const char* fn = "mmf_w2v_mask_drop";
  MmfItemDrop dr;
  if (int rc = mmf_item_drop_fill(fn, p, rng_state, site, item0, &dr)) return rc;
  if (!x_bf16 || !out_bf16 || d <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: null operand or d=%d", fn, d);
  if (int rc = mask_geometry(fn, items, T, starts ? S_max : 1, starts ? length : 1)) return rc;
  if (!starts && dr.thresh == 0u) MMF_FAIL(MMF_E_SHAPE, "%s: neither spans nor dropout: nothing to do", fn);
  if ((d & 7) || (int64_t)T * d > ((int64_t)1 << 32)) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: d=%d (a multiple of 8), T * d = %lld (at most 2^32)", fn, d, (long long)T * d);
  if (!mmf_aligned16(x_bf16) || !mmf_aligned16(out_bf16) || (reinterpret_cast<uintptr_t>(embed) & 3u) || (reinterpret_cast<uintptr_t>(starts) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "%s: x / out must be 16-byte aligned, embed / starts 4-byte aligned", fn);
  const unsigned d8 = (unsigned)d >> 3;
  const dim3 grid((unsigned)mmf_stream_grid((int64_t)T * d8, W2V_THREADS), (unsigned)(items < 65535 ? items : 65535));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned short* x = static_cast<const unsigned short*>(x_bf16);
  unsigned short* out = static_cast<unsigned short*>(out_bf16);
  if (embed) hipLaunchKernelGGL(w2v_mask_drop_kernel<true>, grid, dim3(W2V_THREADS), 0, s, x, embed, starts, out, (unsigned)items, (unsigned)T, d8, S_max, length, dr);
  else       hipLaunchKernelGGL(w2v_mask_drop_kernel<false>, grid, dim3(W2V_THREADS), 0, s, x, embed, starts, out, (unsigned)items, (unsigned)T, d8, S_max, length, dr);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_w2v_mask_embed_grad(const void* dx_bf16, const int* starts, float* partial, int64_t items, int T, int d, int S_max, int length,
                                       int slabs, void* stream) {
  const char* fn = "mmf_w2v_mask_embed_grad";
  if (!dx_bf16 || !starts || !partial || d <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: null operand or d=%d", fn, d);
  if (int rc = mask_geometry(fn, items, T, S_max, length)) return rc;
  const int64_t rows = items * T;
  if (rows >= ((int64_t)1 << 31) || slabs < 1 || slabs > MMF_SUM_SLABS_MAX || slabs > rows)
    MMF_FAIL(MMF_E_SHAPE, "%s: rows=%lld (below 2^31), slabs=%d (1 .. %d, at most the rows)", fn, (long long)rows, slabs, MMF_SUM_SLABS_MAX);
  if ((reinterpret_cast<uintptr_t>(dx_bf16) & 1u) || (reinterpret_cast<uintptr_t>(starts) & 3u) || (reinterpret_cast<uintptr_t>(partial) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "%s: dx must be 2-byte aligned, starts / partial 4-byte aligned", fn);
  const int per = (int)((rows + slabs - 1) / slabs);
  hipLaunchKernelGGL(w2v_mask_embed_grad_kernel, dim3((d + W2V_THREADS - 1) / W2V_THREADS, slabs), dim3(W2V_THREADS), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(dx_bf16), starts, partial, (int)rows, T, d, S_max, length, per);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}
