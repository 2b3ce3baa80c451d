// Whisper's front end (mmfusion/whisper.py): waveform -> log-mel features -> the two padded convolutions' window forms.
//   logmel            HuggingFace WhisperFeatureExtractor's input_features on the device, two launches:
//                       pass 1  a workgroup owns 64 frames of one clip: their samples (zero / reflect padding applied) staged once in
//                               LDS, the 400-point DFT as an f32-input MFMA product against the host's cos | sin table, |X|^2, the
//                               mel filter bank over each filter's run of non-zero bins, log10 -> raw (N, Tm, n_mels) f32 and the
//                               workgroup's maximum
//                       pass 2  the clip's maximum from its workgroups' maxima, the clamp and the scaling -> features (N, n_mels, Tm)
//                               f32 and / or conv1's window form (N, Tm, Kw) bf16
//   feature_window    pass 2's window form from features somebody else made (the same bits as logmel's own window)
//   gelu_window       bias + GELU + the (T_out, k*C) window form of a zero-padded convolution (wav2vec2.hip's gelu_window with a bias
//                     and padding; that kernel keeps its own body and its bits)
//   stem_out          bias + GELU + the position row: the residual stream's first value
// No atomics anywhere and every sum has a fixed order: the same bits on every run.
#include "mmf_internal.h"

namespace {

constexpr int WH_NFFT = 400, WH_HOP = 160, WH_BINS = 201, WH_REFLECT = 200;
constexpr int WH_FT = 64;                                       // frames per pass-1 workgroup: two 32-row MFMA tiles
constexpr int WH_WAVES = MMF_WHISPER_DFT_COLS / 32;              // 7 waves, one 32-bin column tile each (cos and sin)
constexpr int WH_THREADS1 = WH_WAVES * 64;
constexpr int WH_SAMPLES = (WH_FT - 1) * WH_HOP + WH_NFFT;      // samples 64 frames span: adjacent frames share 240 of 400
constexpr int WH_PLD = 225;                                     // row stride of the power tile (201 bins, odd)
constexpr int WH_LDS = WH_FT * WH_PLD;                          // floats: the power tile takes the staged samples' place
constexpr int WH_FT2 = 32, WH_THREADS2 = 256;                   // pass 2: frames per workgroup
constexpr int WH_MAX_MELS = 128;
constexpr float WH_FLOOR = 1e-10f;

static_assert(WH_SAMPLES + WH_SAMPLES / WH_HOP + 1 <= WH_LDS, "the skewed samples fit under the power tile");

// where sample s of the staged run sits: one float of skew per hop, so that the 32 frames an MFMA A fragment reads at one k
// (s = 160 frame + k) fall into 32 different banks
__device__ __forceinline__ int wh_skew(int s) { return s + s / WH_HOP; }

__global__ __launch_bounds__(WH_THREADS1)
void whisper_logmel_pass1_kernel(const float* __restrict__ wave, long long ld, const float* __restrict__ window,
                                 const float* __restrict__ dft, const float* __restrict__ fb, float* __restrict__ raw,
                                 float* __restrict__ blockmax, int L, int n_samples, int n_mels, int Tm) {
  __shared__ float lds[WH_LDS];
  __shared__ float win_s[WH_NFFT];
  __shared__ int lo_s[WH_MAX_MELS], hi_s[WH_MAX_MELS];
  __shared__ float red[WH_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int n = blockIdx.y, t0 = blockIdx.x * WH_FT;
  const float* __restrict__ x = wave + (size_t)n * ld;

  // the samples of frames t0 .. t0 + 63 of the padded clip: zeros behind L, 200 reflected samples on both sides of n_samples
  const long long j0 = (long long)t0 * WH_HOP;
  for (int i = tid; i < WH_SAMPLES; i += WH_THREADS1) {
    const long long j = j0 + i;
    long long o = j - WH_REFLECT;
    if (o < 0) o = -o;
    if (o >= n_samples) o = 2LL * (n_samples - 1) - o;
    lds[wh_skew(i)] = (j < (long long)n_samples + 2 * WH_REFLECT && o >= 0 && o < L) ? x[o] : 0.0f;
  }
  for (int i = tid; i < WH_NFFT; i += WH_THREADS1) win_s[i] = window[i];
  // every filter's run of non-zero bins [lo, hi): the mel product below walks that run only
  if (tid < n_mels) {
    int lo = WH_BINS, hi = 0;
    for (int f = 0; f < WH_BINS; ++f)
      if (fb[f * n_mels + tid] != 0.0f) { lo = f < lo ? f : lo; hi = f + 1; }
    lo_s[tid] = lo; hi_s[tid] = hi;
  }
  __syncthreads();

  // X[frame][bin] = sum_k (x w)[frame][k] (cos | sin)(2 pi bin k / 400): v_mfma_f32_32x32x2_f32, an f32 fmaf chain in k order
  f32x16_t re[2], im[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) re[m][r] = im[m][r] = 0.0f;
  const float* __restrict__ tab = dft + wv * 32 + li;
  const int f0 = li * (WH_HOP + 1), f1 = (li + 32) * (WH_HOP + 1);
#pragma unroll 4
  for (int k = 0; k < WH_NFFT; k += 2) {
    const int kk = k + lk, ks = kk + kk / WH_HOP;
    const float w = win_s[kk];
    const float bc = tab[(size_t)kk * (2 * MMF_WHISPER_DFT_COLS)], bs = tab[(size_t)kk * (2 * MMF_WHISPER_DFT_COLS) + MMF_WHISPER_DFT_COLS];
    const float a0 = lds[f0 + ks] * w, a1 = lds[f1 + ks] * w;
    re[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bc, re[0], 0, 0, 0);
    im[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bs, im[0], 0, 0, 0);
    re[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bc, re[1], 0, 0, 0);
    im[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bs, im[1], 0, 0, 0);
  }
  __syncthreads();                                     // every wave is done with the samples: the power tile takes their place
  const int bin = wv * 32 + li;
  if (bin < WH_BINS) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        lds[row * WH_PLD + bin] = fmaf(re[m][r], re[m][r], im[m][r] * im[m][r]);
      }
  }
  __syncthreads();

  // mel = power . filter over the filter's run, log10 with the floor; the workgroup's maximum over its frames below Tm
  float best = -INFINITY;
  const int frames = Tm - t0 < WH_FT ? Tm - t0 : WH_FT;
  for (int e = tid; e < frames * n_mels; e += WH_THREADS1) {
    const int f = e / n_mels, m = e - f * n_mels;
    const float* __restrict__ p = lds + f * WH_PLD;
    float acc = 0.0f;
    for (int b = lo_s[m]; b < hi_s[m]; ++b) acc = fmaf(p[b], fb[b * n_mels + m], acc);
    const float v = acc > WH_FLOOR ? log10f(acc) : -10.0f;      // log10(max(mel, 1e-10)); the floor's own value is exact
    raw[((size_t)n * Tm + t0 + f) * n_mels + m] = v;
    best = fmaxf(best, v);
  }
  best = wave_max(best);
  if (lane == 0) red[wv] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WH_WAVES; ++w) best = fmaxf(best, red[w]);
    blockmax[(size_t)n * gridDim.x + blockIdx.x] = best;
  }
}

// pass 2.  RAW: src = raw (N, Tm, n_mels), v = (max(raw, clip maximum - 8) + 4) / 4.  Else src = features (N, n_mels, Tm), taken as
// they are.  A workgroup owns 32 frames and holds them with one frame on either side (zeros outside the clip: conv1's padding)
template <bool RAW>
__global__ __launch_bounds__(WH_THREADS2)
void whisper_logmel_pass2_kernel(const float* __restrict__ src, const float* __restrict__ blockmax, int nblk,
                                 float* __restrict__ features, unsigned* __restrict__ window, int n_mels, int Tm, int Kw) {
  __shared__ float tile[(WH_FT2 + 2) * (WH_MAX_MELS + 1)];
  __shared__ float red[WH_THREADS2 / 64];
  const int tid = threadIdx.x, n = blockIdx.y, t0 = blockIdx.x * WH_FT2, S = n_mels + 1;
  float floor_v = 0.0f;
  if (RAW) {
    float best = -INFINITY;
    for (int i = tid; i < nblk; i += WH_THREADS2) best = fmaxf(best, blockmax[(size_t)n * nblk + i]);
    best = wave_max(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    floor_v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) - 8.0f;
  }
  const int rows = WH_FT2 + 2;
  if (RAW) {
    for (int e = tid; e < rows * n_mels; e += WH_THREADS2) {
      const int r = e / n_mels, c = e - r * n_mels, t = t0 - 1 + r;
      tile[r * S + c] = (t >= 0 && t < Tm) ? (fmaxf(src[((size_t)n * Tm + t) * n_mels + c], floor_v) + 4.0f) * 0.25f : 0.0f;
    }
  } else {
    for (int e = tid; e < rows * n_mels; e += WH_THREADS2) {
      const int c = e / rows, r = e - c * rows, t = t0 - 1 + r;
      tile[r * S + c] = (t >= 0 && t < Tm) ? src[((size_t)n * n_mels + c) * Tm + t] : 0.0f;
    }
  }
  __syncthreads();
  const int frames = Tm - t0 < WH_FT2 ? Tm - t0 : WH_FT2;
  if (features) {
    for (int e = tid; e < n_mels * WH_FT2; e += WH_THREADS2) {
      const int c = e / WH_FT2, tt = e - c * WH_FT2;
      if (tt < frames) features[((size_t)n * n_mels + c) * Tm + t0 + tt] = tile[(tt + 1) * S + c];
    }
  }
  if (window) {                                        // row t: frames t - 1, t, t + 1, then zero columns up to Kw; two bf16 a store
    const int pairs = Kw >> 1, live = 3 * n_mels;
    for (int e = tid; e < frames * pairs; e += WH_THREADS2) {
      const int tt = e / pairs, q = (e - tt * pairs) * 2;
      unsigned v = 0u;
      if (q < live) {
        const int j = q / n_mels, c = q - j * n_mels;
        const float* __restrict__ p = tile + (tt + j) * S + c;
        v = pack_bf16x2(p[0], p[1]);
      }
      window[((size_t)n * Tm + t0 + tt) * pairs + (q >> 1)] = v;
    }
  }
}

// ---- bias + GELU + window form of a zero-padded convolution ----------------------------------------------------------------
// The lanes walk the OUTPUT in order; a lane's 8 columns are 8 consecutive channels of one input row (or zeros outside the clip).
__global__ __launch_bounds__(256)
void whisper_gelu_window_kernel(const unsigned short* __restrict__ x, const float* __restrict__ bias, unsigned short* __restrict__ out,
                                int T_in, int C, int k, int s, int pad, unsigned cv /* C/8 */, unsigned nvec /* T_out*k*C/8 */) {
  const unsigned short* __restrict__ src = x + (size_t)blockIdx.y * T_in * C;
  unsigned short* __restrict__ dst = out + (size_t)blockIdx.y * nvec * 8;
  const unsigned rowv = cv * (unsigned)k, stride = gridDim.x * 256;
  for (unsigned v = blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const unsigned t = v / rowv, r = v - t * rowv;
    const unsigned j = r / cv, c = (r - j * cv) << 3;
    const long long f = (long long)t * s + j - pad;
    u32x4_t pk = {0u, 0u, 0u, 0u};
    if (f >= 0 && f < T_in) {
      float a[8];
      unpack8(*reinterpret_cast<const u32x4_t*>(src + (size_t)f * C + c), a);
      const float4 b0 = ld4(bias + c), b1 = ld4(bias + c + 4);
      const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = gelu_erf(a[e] + b[e]);
      pk = pack8(a);
    }
    *reinterpret_cast<u32x4_t*>(dst + (size_t)v * 8) = pk;
  }
}

// out[r][c] = bf16(gelu(x[r][c] + bias[c]) + pos[r % T][c]); a lane reads its 8 values before it writes them: out may be x
__global__ __launch_bounds__(256)
void whisper_stem_out_kernel(const unsigned short* x, const float* __restrict__ bias, const float* __restrict__ pos,
                             unsigned short* out, int T, unsigned dv /* d/8 */, long long nvec) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long long row = v / dv;
    const int c = (int)(v - row * dv) << 3, t = (int)(row % T);
    float a[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(x + v * 8), a);
    const float4 b0 = ld4(bias + c), b1 = ld4(bias + c + 4);
    const float4 p0 = ld4(pos + (size_t)t * dv * 8 + c), p1 = ld4(pos + (size_t)t * dv * 8 + c + 4);
    const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const float p[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = gelu_erf(a[e] + b[e]) + p[e];
    *reinterpret_cast<u32x4_t*>(out + v * 8) = pack8(a);
  }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the window form's checks, shared by the two entries that write one
int window_check(const char* fn, const void* window_bf16, int n_mels, int Kw) {
  if (Kw < 3 * n_mels || (Kw & 7)) MMF_FAIL(MMF_E_SHAPE, "%s: Kw=%d must be a multiple of 8 of at least 3 n_mels = %d", fn, Kw, 3 * n_mels);
  if (!mmf_aligned16(window_bf16)) MMF_FAIL(MMF_E_ALIGN, "%s: window must be 16-byte aligned", fn);
  return MMF_OK;
}

}  // namespace

extern "C" size_t mmf_whisper_logmel_scratch_bytes(int N, int n_samples, int n_mels) {
  if (N <= 0 || n_samples <= 0 || n_mels <= 0) return 0;
  const size_t Tm = (size_t)n_samples / WH_HOP, nblk = (Tm + WH_FT - 1) / WH_FT;
  return ((size_t)N * Tm * n_mels + (size_t)N * nblk) * sizeof(float);
}

extern "C" int mmf_whisper_logmel(const float* wave, int64_t ld, const float* window, const float* dft, const float* mel_fb,
                                  float* features, void* window_bf16, void* scratch, size_t scratch_bytes, int N, int L,
                                  int n_samples, int n_mels, int Kw, void* stream) {
  const char* fn = "mmf_whisper_logmel";
  if (!wave || !window || !dft || !mel_fb || !scratch || (!features && !window_bf16))
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand (features and window may not both be NULL)", fn);
  if (N <= 0 || n_samples <= 0 || n_samples % 320 || L < 1 || L > n_samples || ld < L)
    MMF_FAIL(MMF_E_SHAPE, "%s: N=%d, L=%d in 1 .. n_samples=%d (a multiple of 320), ld=%lld >= L", fn, N, L, n_samples, (long long)ld);
  if ((n_mels != 80 && n_mels != 128) || N > 65535)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: n_mels=%d (80 or 128), N=%d (at most 65535)", fn, n_mels, N);
  if (window_bf16) if (int rc = window_check(fn, window_bf16, n_mels, Kw)) return rc;
  if (scratch_bytes < mmf_whisper_logmel_scratch_bytes(N, n_samples, n_mels))
    MMF_FAIL(MMF_E_SHAPE, "%s: scratch holds %zu bytes, mmf_whisper_logmel_scratch_bytes asks for %zu", fn, scratch_bytes,
             mmf_whisper_logmel_scratch_bytes(N, n_samples, n_mels));
  if (!aligned4(wave) || !aligned4(window) || !aligned4(dft) || !aligned4(mel_fb) || !aligned4(features) || !mmf_aligned16(scratch))
    MMF_FAIL(MMF_E_ALIGN, "%s: the f32 operands must be 4-byte aligned, scratch 16-byte aligned", fn);
  const int Tm = n_samples / WH_HOP, nblk = (Tm + WH_FT - 1) / WH_FT;
  float* raw = static_cast<float*>(scratch);
  float* blockmax = raw + (size_t)N * Tm * n_mels;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(whisper_logmel_pass1_kernel, dim3(nblk, N), dim3(WH_THREADS1), 0, s, wave, (long long)ld, window, dft, mel_fb, raw,
                     blockmax, L, n_samples, n_mels, Tm);
  MMF_CHECK_LAUNCH("mmf_whisper_logmel(pass 1)");
  hipLaunchKernelGGL(whisper_logmel_pass2_kernel<true>, dim3((Tm + WH_FT2 - 1) / WH_FT2, N), dim3(WH_THREADS2), 0, s, raw, blockmax, nblk,
                     features, static_cast<unsigned*>(window_bf16), n_mels, Tm, Kw);
  MMF_CHECK_LAUNCH("mmf_whisper_logmel(pass 2)");
  return MMF_OK;
}

extern "C" int mmf_whisper_feature_window(const float* features, void* window_bf16, int N, int n_mels, int Tm, int Kw, void* stream) {
  const char* fn = "mmf_whisper_feature_window";
  if (!features || !window_bf16 || N <= 0 || Tm <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: null operand or N=%d Tm=%d", fn, N, Tm);
  if ((n_mels != 80 && n_mels != 128) || N > 65535)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: n_mels=%d (80 or 128), N=%d (at most 65535)", fn, n_mels, N);
  if (int rc = window_check(fn, window_bf16, n_mels, Kw)) return rc;
  if (!aligned4(features)) MMF_FAIL(MMF_E_ALIGN, "%s: features must be 4-byte aligned", fn);
  hipLaunchKernelGGL(whisper_logmel_pass2_kernel<false>, dim3((Tm + WH_FT2 - 1) / WH_FT2, N), dim3(WH_THREADS2), 0,
                     static_cast<hipStream_t>(stream), features, static_cast<const float*>(nullptr), 0, static_cast<float*>(nullptr),
                     static_cast<unsigned*>(window_bf16), n_mels, Tm, Kw);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_whisper_gelu_window(const void* x_bf16, const float* bias, void* out_bf16, int N, int T_in, int C, int k, int s,
                                       int pad, void* stream) {
  const char* fn = "mmf_whisper_gelu_window";
  if (!x_bf16 || !bias || !out_bf16 || N <= 0 || T_in <= 0 || C <= 0 || k <= 0 || s <= 0 || pad < 0)
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or N=%d T_in=%d C=%d k=%d s=%d pad=%d", fn, N, T_in, C, k, s, pad);
  if (pad >= k || T_in + 2 * (int64_t)pad < k)
    MMF_FAIL(MMF_E_SHAPE, "%s: pad=%d must be below k=%d, and T_in + 2 pad = %lld at least k", fn, pad, k, (long long)T_in + 2 * pad);
  const int64_t T_out = (T_in + 2 * (int64_t)pad - k) / s + 1, nvec = T_out * k * (C / 8);
  if ((C & 7) || N > 65535 || nvec >= (int64_t)1 << 31 || x_bf16 == out_bf16)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: C=%d (multiple of 8), N=%d (at most 65535), %lld output elements per clip (below 2^34), "
             "out must not be x", fn, C, N, (long long)nvec * 8);
  if (!mmf_aligned16(x_bf16) || !mmf_aligned16(out_bf16) || !mmf_aligned16(bias))
    MMF_FAIL(MMF_E_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  hipLaunchKernelGGL(whisper_gelu_window_kernel, dim3(mmf_stream_grid(nvec, 256), N), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(x_bf16), bias, static_cast<unsigned short*>(out_bf16), T_in, C, k, s, pad,
                     (unsigned)(C / 8), (unsigned)nvec);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_whisper_stem_out(const void* x_bf16, const float* bias, const float* pos, void* out_bf16, int64_t rows, int T, int d,
                                    void* stream) {
  const char* fn = "mmf_whisper_stem_out";
  if (!x_bf16 || !bias || !pos || !out_bf16 || rows <= 0 || T <= 0 || d <= 0 || rows % T)
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand, or rows=%lld not a positive multiple of T=%d, or d=%d", fn, (long long)rows, T, d);
  if ((d & 7) || rows > ((int64_t)1 << 40) / d) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: d=%d (multiple of 8), rows d below 2^40", fn, d);
  if (!mmf_aligned16(x_bf16) || !mmf_aligned16(out_bf16) || !mmf_aligned16(bias) || !mmf_aligned16(pos))
    MMF_FAIL(MMF_E_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  const int64_t nvec = rows * (d / 8);
  hipLaunchKernelGGL(whisper_stem_out_kernel, dim3(mmf_stream_grid(nvec, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(x_bf16), bias, pos, static_cast<unsigned short*>(out_bf16), T, (unsigned)(d / 8),
                     (long long)nvec);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}
