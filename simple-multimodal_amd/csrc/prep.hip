// Input preparation on the device (mmfusion/prep.py; the reference does this per sample on the host, data/dataset_loaders.py:95-261):
// decoded uint8 frames -> the ViT's f32 pixels or straight its bf16 patch matrix (resize, /255, HWC -> CHW, brightness, flip), and
// f32 PCM -> the Wav2Vec2 waveform (mono mix, rational resampling, pad / truncate; additive noise and time stretch).  All three are
// streaming / short-FIR kernels with blockIdx.y = frame / clip: one 16-byte store per lane on the video side, one f32 per lane on
// the audio side (an audio output costs tens of taps, its store is not what bounds it).
// Coordinates are integers throughout: a source index and its fraction are quotient and remainder of one
// integer division, so the geometry is exact at any size and both video forms see the same f32 value.
#include "mmf_internal.h"

namespace {

constexpr int PREP_THREADS = 256;
constexpr int PREP_MAX_SIDE = 16384;                       // (2 x + 1) * side stays below 2^31
constexpr int PREP_ROWS = 8;                               // output rows of a video tile (it is PREP_THREADS columns wide)
constexpr int PREP_LDS_FLOATS = 12288;                     // the resampler's tile form: 48 KiB of LDS per workgroup at most
constexpr int PREP_TILE_OUT = 1024;                        // ... and about this many outputs per workgroup

// Half-pixel-centre source coordinate of output index `o` on an axis resized `src` -> `dst`: (o + 0.5) * src / dst - 0.5 clamped
// below at 0, as i0 = floor, i1 = min(i0 + 1, src - 1) and the fraction, which is rem / (2 dst) with both exact in f32 (frames:
// 2 dst <= 32768).
struct Tap { int i0, i1; float w; };
__device__ __forceinline__ Tap prep_tap(int o, int src, int dst) {
  const int den = 2 * dst, num = max((2 * o + 1) * src - dst, 0);
  const int i0 = num / den, rem = num - i0 * den;
  return Tap{i0, i0 + 1 < src ? i0 + 1 : src - 1, (float)rem / (float)den};
}

// The value of one output pixel from its four source bytes.  Every multiply-add is an explicit fmaf and nothing else can
// contract, so the f32 form and the patch form compute the same bits whatever surrounds the call.
__device__ __forceinline__ float prep_pixel(const unsigned char* __restrict__ row0, const unsigned char* __restrict__ row1,
                                            const Tap tx, float wy, int ch, float bright) {
  const float a = (float)row0[tx.i0 * 3 + ch], b = (float)row0[tx.i1 * 3 + ch];
  const float c = (float)row1[tx.i0 * 3 + ch], d = (float)row1[tx.i1 * 3 + ch];
  const float top = fmaf(tx.w, b - a, a), bot = fmaf(tx.w, d - c, c);
  const float v = fmaf(wy, bot - top, top);
  return fminf(fmaxf(v * (1.0f / 255.0f) * bright, 0.f), 1.f);
}

// frames (N, Hs, Ws, 3) u8 -> PATCH ? the patch matrix (N * gh * gw, 3 * P * P) bf16 of vit_patchify_kernel (vit.hip) : (N, 3, H, W)
// f32.  blockIdx.y = frame; a workgroup takes tiles of PREP_ROWS output rows x PREP_THREADS output columns in a grid-stride loop.
// In a tile lane t owns COLUMN x0 + t: its horizontal taps are formed once, the vertical ones are uniform, and the three channel
// bytes of a tap are neighbours, so a wave's load touches the few cache lines under 64 neighbouring columns of one source row
// (with 8 consecutive pixels per lane and one load per pixel, the first form, a wave load touched up to 64 lines and the kernel
// ran at 1 TB/s: DESIGN.md section 11).  The values go through LDS and leave as one 16-byte store per lane, 8 px (bf16) or 4 (f32).
template <bool PATCH>
__global__ __launch_bounds__(PREP_THREADS)
void video_prepare_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ live,
                          const float* __restrict__ brightness, const unsigned char* __restrict__ flip, void* __restrict__ out,
                          int Hs, int Ws, int H, int W, int P, int bgr) {
  constexpr int PX = PATCH ? 8 : 4;
  __shared__ __attribute__((aligned(16))) float vals[PREP_ROWS][3][PREP_THREADS];
  const unsigned n = blockIdx.y, tid = threadIdx.x;
  const unsigned char* __restrict__ img = frames + (size_t)n * Hs * Ws * 3;
  const bool dead = live && !live[n];                      // uniform over the workgroup
  const bool flipped = flip && flip[n];
  const float bright = brightness ? brightness[n] : 1.0f;
  const int xtiles = (W + PREP_THREADS - 1) / PREP_THREADS, units = ((H + PREP_ROWS - 1) / PREP_ROWS) * xtiles;
  for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int y0 = (unit / xtiles) * PREP_ROWS, x0 = (unit % xtiles) * PREP_THREADS;
    const int rows = min(PREP_ROWS, H - y0), cols = min(PREP_THREADS, W - x0);
    if (!dead && (int)tid < cols) {
      const int x = x0 + (int)tid;
      const Tap tx = prep_tap(flipped ? W - 1 - x : x, Ws, W);
      for (int r = 0; r < rows; ++r) {
        const Tap ty = prep_tap(y0 + r, Hs, H);
        const unsigned char* __restrict__ row0 = img + (size_t)ty.i0 * Ws * 3;
        const unsigned char* __restrict__ row1 = img + (size_t)ty.i1 * Ws * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) vals[r][c][tid] = prep_pixel(row0, row1, tx, ty.w, bgr ? 2 - c : c, bright);
      }
    }
    __syncthreads();
    const int cv = cols / PX, nvec = rows * 3 * cv;        // cols is a multiple of PX: W and the tile width are
    for (int v = tid; v < nvec; v += PREP_THREADS) {
      const int rc = v / cv, xl = (v - rc * cv) * PX, r = rc / 3, c = rc - r * 3;
      const int y = y0 + r, x = x0 + xl;
      f32x4_t a = {0.f, 0.f, 0.f, 0.f}, b = a;
      if (!dead) {
        a = *reinterpret_cast<const f32x4_t*>(&vals[r][c][xl]);
        if constexpr (PATCH) b = *reinterpret_cast<const f32x4_t*>(&vals[r][c][xl + 4]);
      }
      if constexpr (PATCH) {
        const int gy = y / P, gx = x / P;
        const size_t at = (((size_t)n * (H / P) + gy) * (W / P) + gx) * (3 * P * P) + (size_t)(c * P + (y - gy * P)) * P + (x - gx * P);
        *reinterpret_cast<u32x4_t*>(static_cast<unsigned short*>(out) + at) = pack8(a, b);
      } else {
        *reinterpret_cast<f32x4_t*>(static_cast<float*>(out) + (((size_t)n * 3 + c) * H + y) * W + x) = a;
      }
    }
    __syncthreads();                                       // the next tile overwrites vals
  }
}

// wave (B, C, Ls) f32 -> out (B, L) f32: mono mean, polyphase windowed-sinc resampling orig -> new, zero past the clip's resampled
// length.  Output m = i * new + j reads x[i * orig + k - width] against table[j][k]; of the 2 width + orig columns of a table row
// only k in (orig j / new, orig j / new + 2 width] can be non-zero (the filter's support is at most width on either side of the
// phase's centre width + orig j / new), so those 2 width taps are all that is read.  A null table is orig == new: one unit tap.
// The direct form, straight from memory: it serves equal rates (a copy) and filters too long for the tile form below.  For
// neighbouring lanes the taps of table[j] lie a row apart, 64 cache lines per wave load, which is what bounds it.
__global__ __launch_bounds__(PREP_THREADS)
void audio_resample_kernel(const float* __restrict__ wave, const int* __restrict__ len, const float* __restrict__ table,
                           float* __restrict__ out, int C, int Ls, int L, int orig, int new_, int width) {
  const unsigned b = blockIdx.y;
  const float* __restrict__ x = wave + (size_t)b * C * Ls;
  float* __restrict__ dst = out + (size_t)b * L;
  int n_in = len ? len[b] : Ls;
  n_in = n_in < 0 ? 0 : (n_in > Ls ? Ls : n_in);
  const long long n_out = ((long long)new_ * n_in + orig - 1) / orig;
  const float inv_c = 1.0f / (float)C;
  const int K = 2 * width + orig;
  const unsigned stride = gridDim.x * PREP_THREADS;
  for (unsigned m = blockIdx.x * PREP_THREADS + threadIdx.x; m < (unsigned)L; m += stride) {
    float acc = 0.f;
    if ((long long)m < n_out) {
      if (!table) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += x[(size_t)c * Ls + m];
        acc = s * inv_c;
      } else {
        const int i = (int)(m / (unsigned)new_), j = (int)m - i * new_;
        const int k_lo = (int)((long long)orig * j / new_) + 1;
        const long long base = (long long)i * orig - width;
        const float* __restrict__ trow = table + (size_t)j * K;
        for (int k = k_lo; k < k_lo + 2 * width; ++k) {               // k <= orig - 1 + 2 width: inside the row
          const long long src = base + k;
          if (src < 0 || src >= n_in) continue;
          float s = 0.f;
          for (int c = 0; c < C; ++c) s += x[(size_t)c * Ls + src];
          acc = fmaf(s * inv_c, trow[k], acc);
        }
      }
    }
    dst[m] = acc;
  }
}

// The tile form: a workgroup owns IB input blocks of one clip, i in [i0, i0 + IB), i.e. IB * new consecutive outputs of every
// phase.  It stages in LDS what they read: xs, the IB * orig + 2 width mono samples from i0 * orig - width on (0 outside the clip:
// mixed once, not once per tap), and ts, the 2 width live taps of every phase packed (new, 2 width).  Then output (i, j) is
// sum_t xs[(i - i0) orig + k_lo(j) + t] * ts[j][t].  LDS floats: IB * orig + 2 width + new * 2 width (the host picks IB).
__global__ __launch_bounds__(PREP_THREADS)
void audio_resample_tile_kernel(const float* __restrict__ wave, const int* __restrict__ len, const float* __restrict__ table,
                                float* __restrict__ out, int C, int Ls, int L, int orig, int new_, int width, int IB) {
  extern __shared__ float prep_lds[];
  const unsigned b = blockIdx.y;
  const float* __restrict__ x = wave + (size_t)b * C * Ls;
  float* __restrict__ dst = out + (size_t)b * L;
  int n_in = len ? len[b] : Ls;
  n_in = n_in < 0 ? 0 : (n_in > Ls ? Ls : n_in);
  const long long n_out = ((long long)new_ * n_in + orig - 1) / orig;
  const int taps = 2 * width, K = taps + orig, n_xs = IB * orig + taps, n_tile = IB * new_;
  const long long m0 = (long long)blockIdx.x * n_tile;              // first output of the tile; m0 < L by the grid
  const int n_store = (int)(L - m0 < n_tile ? L - m0 : n_tile);
  if (m0 >= n_out) {                                                // the whole tile lies past the clip's end (uniform)
    for (int r = threadIdx.x; r < n_store; r += PREP_THREADS) dst[m0 + r] = 0.f;
    return;
  }
  float* __restrict__ xs = prep_lds;
  float* __restrict__ ts = prep_lds + n_xs;
  const long long x0 = (long long)blockIdx.x * IB * orig - width;
  const float inv_c = 1.0f / (float)C;
  for (int r = threadIdx.x; r < n_xs; r += PREP_THREADS) {
    const long long src = x0 + r;
    float s = 0.f;
    if (src >= 0 && src < n_in)
      for (int c = 0; c < C; ++c) s += x[(size_t)c * Ls + src];
    xs[r] = s * inv_c;
  }
  for (int r = threadIdx.x; r < new_ * taps; r += PREP_THREADS) {
    const int j = r / taps, t = r - j * taps;
    ts[r] = table[(size_t)j * K + (int)((long long)orig * j / new_) + 1 + t];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < n_store; r += PREP_THREADS) {
    float acc = 0.f;
    if (m0 + r < n_out) {
      const int i = r / new_, j = r - i * new_;
      const float* __restrict__ xp = xs + i * orig + (int)((long long)orig * j / new_) + 1;
      const float* __restrict__ tp = ts + j * taps;
      for (int t = 0; t < taps; ++t) acc = fmaf(xp[t], tp[t], acc);
    }
    dst[m0 + r] = acc;
  }
}

// standard normal for (key, j): Box-Muller from draws 2 j and 2 j + 1 of the counter hash; the top 24 bits of a draw are its
// unit value, (0, 1] under the logarithm and [0, 1) in the angle.
__device__ __forceinline__ float prep_normal(unsigned key, unsigned j) {
  const unsigned u1 = mmf_mix32(key + (2u * j) * 0x9E3779B9u), u2 = mmf_mix32(key + (2u * j + 1u) * 0x9E3779B9u);
  const float f1 = (float)((u1 >> 8) + 1u) * 0x1p-24f, f2 = (float)(u2 >> 8) * 0x1p-24f;
  return sqrtf(-2.0f * logf(f1)) * cosf(6.28318530717958647692f * f2);
}

// x (B, L) f32 -> out (B, L) f32: xn = x + 0.01 z where the clip's noise is on, then the first min(stretch_len, L) outputs are
// xn resized L -> stretch_len by linear interpolation (half-sample centres, as prep_tap but in 64 bits) and the rest is 0.
__global__ __launch_bounds__(PREP_THREADS)
void audio_augment_kernel(const float* __restrict__ x, float* __restrict__ out, const unsigned char* __restrict__ noise_on,
                          const int* __restrict__ stretch_len, const unsigned long long* __restrict__ state, unsigned site, int L) {
  const unsigned b = blockIdx.y;
  const float* __restrict__ src = x + (size_t)b * L;
  float* __restrict__ dst = out + (size_t)b * L;
  const bool noisy = noise_on && noise_on[b];
  const unsigned key = noisy ? mmf_rng_key(*state, site, b) : 0u;
  int sl = stretch_len ? stretch_len[b] : L;
  if (sl < 1) sl = L;
  const unsigned n_live = (unsigned)(sl < L ? sl : L);
  const long long den = 2ll * sl;
  const unsigned stride = gridDim.x * PREP_THREADS;
  for (unsigned i = blockIdx.x * PREP_THREADS + threadIdx.x; i < (unsigned)L; i += stride) {
    float r = 0.f;
    if (i < n_live) {
      const long long num = (2ll * i + 1) * L - sl;
      unsigned j0 = 0;
      float w = 0.f;
      if (num > 0) {
        j0 = (unsigned)(num / den);
        w = (float)(num - (long long)j0 * den) / (float)den;     // both exact below 2^24, else rounded: 2^-24 relative in w
      }
      const unsigned j1 = j0 + 1 < (unsigned)L ? j0 + 1 : (unsigned)L - 1;
      float a = src[j0], c = src[j1];
      if (noisy) {
        a = fmaf(0.01f, prep_normal(key, j0), a);
        c = fmaf(0.01f, prep_normal(key, j1), c);
      }
      r = fmaf(w, c - a, a);
    }
    dst[i] = r;
  }
}

// both forms: patch selects the bf16 patch matrix (P its patch size), else the f32 pixels
int video_prepare(const char* who, bool patch, const uint8_t* frames, const uint8_t* live, const float* brightness, const uint8_t* flip,
                  void* out, int N, int Hs, int Ws, int H, int W, int P, int bgr, void* stream) {
  if (!frames || !out || N <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0)
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or N=%d Hs=%d Ws=%d H=%d W=%d", who, N, Hs, Ws, H, W);
  if (patch && P <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: P=%d", who, P);
  if (patch && ((P & 7) || H % P || W % P))
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: H=%d W=%d P=%d (needs P %% 8 == 0, H %% P == 0, W %% P == 0)", who, H, W, P);
  if (!patch && (W & 3)) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: W=%d must be a multiple of 4", who, W);
  if (N > 65535 || Hs > PREP_MAX_SIDE || Ws > PREP_MAX_SIDE || H > PREP_MAX_SIDE || W > PREP_MAX_SIDE)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: N=%d frames in one call (at most 65535) or a side above %d", who, N, PREP_MAX_SIDE);
  if (!mmf_aligned16(out)) MMF_FAIL(MMF_E_ALIGN, "%s: the output must be 16-byte aligned", who);
  if (brightness && (reinterpret_cast<uintptr_t>(brightness) & 3u)) MMF_FAIL(MMF_E_ALIGN, "%s: brightness must be 4-byte aligned", who);
  const int64_t tiles = (int64_t)((H + PREP_ROWS - 1) / PREP_ROWS) * ((W + PREP_THREADS - 1) / PREP_THREADS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(mmf_stream_grid(tiles * PREP_THREADS, PREP_THREADS), N);
  if (!patch) hipLaunchKernelGGL(video_prepare_kernel<false>, grid, dim3(PREP_THREADS), 0, s, frames, live, brightness, flip, out, Hs, Ws, H, W, 0, bgr);
  else        hipLaunchKernelGGL(video_prepare_kernel<true>, grid, dim3(PREP_THREADS), 0, s, frames, live, brightness, flip, out, Hs, Ws, H, W, P, bgr);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}

}  // namespace

extern "C" int mmf_video_prepare(const uint8_t* frames, const uint8_t* live, const float* brightness, const uint8_t* flip, float* pixels,
                                 int N, int Hs, int Ws, int H, int W, int bgr, void* stream) {
  return video_prepare("mmf_video_prepare", false, frames, live, brightness, flip, pixels, N, Hs, Ws, H, W, 0, bgr, stream);
}

extern "C" int mmf_video_prepare_patches(const uint8_t* frames, const uint8_t* live, const float* brightness, const uint8_t* flip,
                                         void* patches_bf16, int N, int Hs, int Ws, int H, int W, int P, int bgr, void* stream) {
  return video_prepare("mmf_video_prepare_patches", true, frames, live, brightness, flip, patches_bf16, N, Hs, Ws, H, W, P, bgr, stream);
}

extern "C" int mmf_audio_resample(const float* wave, const int* len, const float* table, int64_t table_elems, float* out, int B, int C,
                                  int64_t Ls, int64_t L, int orig, int new_, int width, void* stream) {
  if (!wave || !out || B <= 0 || C <= 0 || Ls <= 0 || L <= 0 || orig <= 0 || new_ <= 0 || width < 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_audio_resample: null operand or B=%d C=%d Ls=%lld L=%lld orig=%d new=%d width=%d", B, C, (long long)Ls,
             (long long)L, orig, new_, width);
  if (orig == new_ ? (table != nullptr) : (!table || orig > (1 << 20) || new_ > (1 << 20)))
    MMF_FAIL(MMF_E_SHAPE, "mmf_audio_resample: orig=%d new=%d takes %s", orig, new_, orig == new_ ? "a null table" : "a table and rates below 2^20");
  if (table) {
    const double base = (orig < new_ ? orig : new_) * 0.99;          // the definition of include/mmfusion.h
    const int want = (int)ceil(6.0 * orig / base);
    if (width != want || table_elems != (int64_t)new_ * (2 * width + orig))
      MMF_FAIL(MMF_E_SHAPE, "mmf_audio_resample: width=%d (the filter has %d) or a table of %lld elements (it has %lld)", width, want,
               (long long)table_elems, (long long)new_ * (2 * want + orig));
  }
  if (B > 65535 || Ls >= (int64_t)1 << 30 || L >= (int64_t)1 << 30 || (int64_t)C * Ls >= (int64_t)1 << 40)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_audio_resample: B=%d (at most 65535), Ls=%lld, L=%lld (below 2^30)", B, (long long)Ls, (long long)L);
  if ((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(len)) & 3u)
    MMF_FAIL(MMF_E_ALIGN, "mmf_audio_resample: pointers must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the tile form where one input block's samples and every phase's live taps fit its LDS budget, with as many blocks per
  // workgroup as fit, up to about PREP_TILE_OUT outputs; else (and for equal rates) the direct form
  const int64_t fixed = table ? 2 * (int64_t)width * (new_ + 1) : 0;
  if (table && fixed + orig <= PREP_LDS_FLOATS) {
    int64_t IB = (PREP_TILE_OUT + new_ - 1) / new_;
    if (IB > (PREP_LDS_FLOATS - fixed) / orig) IB = (PREP_LDS_FLOATS - fixed) / orig;
    const int64_t tiles = (L + IB * new_ - 1) / (IB * new_);
    hipLaunchKernelGGL(audio_resample_tile_kernel, dim3((unsigned)tiles, B), dim3(PREP_THREADS), (size_t)(fixed + IB * orig) * sizeof(float), s,
                       wave, len, table, out, C, (int)Ls, (int)L, orig, new_, width, (int)IB);
  } else {
    hipLaunchKernelGGL(audio_resample_kernel, dim3(mmf_stream_grid(L, PREP_THREADS), B), dim3(PREP_THREADS), 0, s,
                       wave, len, table, out, C, (int)Ls, (int)L, orig, new_, table ? width : 0);
  }
  MMF_CHECK_LAUNCH("mmf_audio_resample");
  return MMF_OK;
}

extern "C" int mmf_audio_augment(const float* x, float* out, const uint8_t* noise_on, const int* stretch_len, const uint64_t* rng_state,
                                 uint32_t site, int B, int64_t L, void* stream) {
  if (!x || !out || B <= 0 || L <= 0 || (noise_on && !rng_state))
    MMF_FAIL(MMF_E_SHAPE, "mmf_audio_augment: null operand (noise needs the RNG state) or B=%d L=%lld", B, (long long)L);
  if (x == out) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_audio_augment: not in place (a stretched output reads its neighbours' inputs)");
  if (B > 65535 || L >= (int64_t)1 << 30) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_audio_augment: B=%d (at most 65535), L=%lld (below 2^30)", B, (long long)L);
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(stretch_len)) & 3u) ||
      (reinterpret_cast<uintptr_t>(rng_state) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "mmf_audio_augment: x / out / stretch_len must be 4-byte and the RNG state 8-byte aligned");
  hipLaunchKernelGGL(audio_augment_kernel, dim3(mmf_stream_grid(L, PREP_THREADS), B), dim3(PREP_THREADS), 0, static_cast<hipStream_t>(stream),
                     x, out, noise_on, stretch_len, reinterpret_cast<const unsigned long long*>(rng_state), site, (int)L);
  MMF_CHECK_LAUNCH("mmf_audio_augment");
  return MMF_OK;
}
