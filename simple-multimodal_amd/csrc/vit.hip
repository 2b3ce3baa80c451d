// The pieces a ViT forward has and the fusion path did not (mmfusion/vit.py): patch extraction for the patch-embedding
// GEMM, CLS / position tokens, exact (erf) GELU (and its backward, for the DeBERTa input gradient).  All are HBM-bound
// streaming kernels: one 16-byte bf16 access (8 elements) per lane on the bf16 side, two 16-byte accesses on the f32 side, grid-stride loops on mmf_stream_grid's
// grid (mmf_internal.h) per grid row.
#include "mmf_internal.h"

namespace {

constexpr int VIT_THREADS = 256;

// (N, C, H, W) f32 -> (N * gh * gw, C * P * P) bf16, column (c, py, px).  blockIdx.y = image; inside an image the lanes
// walk the OUTPUT in order (every wave store covers 1 KiB contiguous); a lane's 8 output columns are 8 consecutive px of
// one pixel row (P % 8 == 0), i.e. 32 contiguous input bytes, and the P / 8 lanes of one patch row read P * 4 contiguous
// bytes.  The other patches of the same pixel row are C * P * P / 8 lanes further on, so the rest of each input cache line is
// fetched by the same or a neighbouring workgroup.
__global__ __launch_bounds__(VIT_THREADS)
void vit_patchify_kernel(const float* __restrict__ pix, unsigned short* __restrict__ out, int C, int H, int W, int P,
                         int gw, unsigned kv /* C*P*P/8 */, unsigned nvec /* gh*gw*kv */) {
  const unsigned pv = (unsigned)P >> 3, ppv = pv * (unsigned)P;      // vectors per patch row / per patch channel
  const float* __restrict__ img = pix + (size_t)blockIdx.y * C * H * W;
  unsigned short* __restrict__ dst = out + (size_t)blockIdx.y * nvec * 8;
  const unsigned stride = gridDim.x * VIT_THREADS;
  for (unsigned v = blockIdx.x * VIT_THREADS + threadIdx.x; v < nvec; v += stride) {
    const unsigned patch = v / kv, k = v - patch * kv;
    const unsigned gy = patch / (unsigned)gw, gx = patch - gy * (unsigned)gw;
    const unsigned c = k / ppv, r = k - c * ppv;
    const unsigned py = r / pv, px = (r - py * pv) << 3;
    const float* __restrict__ src = img + ((size_t)c * H + (gy * P + py)) * W + (gx * P + px);
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(src);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(src + 4);
    *reinterpret_cast<u32x4_t*>(dst + (size_t)v * 8) = pack8(a, b);
  }
}

// tokens[n][0] = cls + pos[0]; tokens[n][1 + p] = patch_emb[n][p] + pos[1 + p]; f32 add, one rounding.  blockIdx.y = image;
// inside an image the flat element index of tokens IS the index into pos, and the one into patch_emb shifted by d.
__global__ __launch_bounds__(VIT_THREADS)
void vit_embed_tokens_kernel(const unsigned short* __restrict__ pe, const float* __restrict__ cls, const float* __restrict__ pos,
                             unsigned short* __restrict__ tok, int T, int d) {
  const unsigned dv = (unsigned)d >> 3, nvec = (unsigned)T * dv;
  const unsigned short* __restrict__ src = pe + (size_t)blockIdx.y * (T - 1) * d;
  unsigned short* __restrict__ dst = tok + (size_t)blockIdx.y * T * d;
  const unsigned stride = gridDim.x * VIT_THREADS;
  for (unsigned v = blockIdx.x * VIT_THREADS + threadIdx.x; v < nvec; v += stride) {
    const f32x4_t p0 = *reinterpret_cast<const f32x4_t*>(pos + (size_t)v * 8);
    const f32x4_t p1 = *reinterpret_cast<const f32x4_t*>(pos + (size_t)v * 8 + 4);
    f32x4_t a, b;
    if (v < dv) {
      a = *reinterpret_cast<const f32x4_t*>(cls + v * 8);
      b = *reinterpret_cast<const f32x4_t*>(cls + v * 8 + 4);
    } else {
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(src + (size_t)(v - dv) * 8);
      a = f32x4_t{bf16lo(w[0]), bf16hi(w[0]), bf16lo(w[1]), bf16hi(w[1])};
      b = f32x4_t{bf16lo(w[2]), bf16hi(w[2]), bf16lo(w[3]), bf16hi(w[3])};
    }
    *reinterpret_cast<u32x4_t*>(dst + (size_t)v * 8) = pack8(a + p0, b + p1);
  }
}

// y <- gelu(x + bias), rows x cols with row stride ld; y may be x (the in-place entry).  nvec = rows * cols / 8 < 2^31 (the host
// splits longer inputs).
template <bool HAS_BIAS>
__global__ __launch_bounds__(VIT_THREADS)
void bias_gelu_kernel(const unsigned short* x, unsigned short* y, const float* __restrict__ bias, unsigned nvec, unsigned cv /* cols/8 */, int ld) {
  const unsigned stride = gridDim.x * VIT_THREADS;
  for (unsigned v = blockIdx.x * VIT_THREADS + threadIdx.x; v < nvec; v += stride) {
    const unsigned r = v / cv, j = (v - r * cv) << 3;
    const u32x4_t w = *reinterpret_cast<const u32x4_t*>(x + (size_t)r * ld + j);
    f32x4_t a = f32x4_t{bf16lo(w[0]), bf16hi(w[0]), bf16lo(w[1]), bf16hi(w[1])};
    f32x4_t b = f32x4_t{bf16lo(w[2]), bf16hi(w[2]), bf16lo(w[3]), bf16hi(w[3])};
    if (HAS_BIAS) {
      a += *reinterpret_cast<const f32x4_t*>(bias + j);
      b += *reinterpret_cast<const f32x4_t*>(bias + j + 4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = gelu_erf(a[e]); b[e] = gelu_erf(b[e]); }
    *reinterpret_cast<u32x4_t*>(y + (size_t)r * ld + j) = pack8(a, b);
  }
}

// dh <- dg * gelu'(h + bias), gelu'(v) = Phi(v) + v phi(v); dh may be dg.  Phi through erfc: 1 + erf(v / sqrt 2) loses every
// digit of Phi in the left tail (v < -5), where v phi(v) is just as small and the derivative would be f32 noise.
__device__ __forceinline__ float gelu_erf_grad(float v) {
  return 0.5f * erfcf(v * -0.70710678118654752440f) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}
template <bool HAS_BIAS>
__global__ __launch_bounds__(VIT_THREADS)
void bias_gelu_bwd_kernel(const unsigned short* dg, const unsigned short* __restrict__ h, const float* __restrict__ bias, unsigned short* dh,
                          unsigned nvec, unsigned cv /* cols/8 */, int ld) {
  const unsigned stride = gridDim.x * VIT_THREADS;
  for (unsigned v = blockIdx.x * VIT_THREADS + threadIdx.x; v < nvec; v += stride) {
    const unsigned r = v / cv, j = (v - r * cv) << 3;
    float x[8], g[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(h + (size_t)r * ld + j), x);
    unpack8(*reinterpret_cast<const u32x4_t*>(dg + (size_t)r * ld + j), g);
    if (HAS_BIAS) {
      const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(bias + j), b1 = *reinterpret_cast<const f32x4_t*>(bias + j + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { x[e] += b0[e]; x[4 + e] += b1[e]; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] *= gelu_erf_grad(x[e]);
    *reinterpret_cast<u32x4_t*>(dh + (size_t)r * ld + j) = pack8(g);
  }
}

// the checks and the row split the three GELU entries share; `launch(first row, vectors)` enqueues one piece
template <typename Launch>
int bias_gelu_run(const char* fn, const void* a, const void* b, const void* c, const float* bias, int64_t rows, int cols, int ld, Launch launch) {
  if (!a || !b || !c || rows <= 0 || cols <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: null operand or rows=%lld cols=%d", fn, (long long)rows, cols);
  if ((cols & 7) || (ld & 7) || ld < cols) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: cols=%d ld=%d (multiples of 8, ld >= cols)", fn, cols, ld);
  if (!mmf_aligned16(a) || !mmf_aligned16(b) || !mmf_aligned16(c) || (bias && !mmf_aligned16(bias))) MMF_FAIL(MMF_E_ALIGN, "%s: pointers must be 16-byte aligned", fn);
  const unsigned cv = (unsigned)cols >> 3;
  const int64_t max_rows = (((int64_t)1 << 31) - 1) / cv;             // rows of one launch: 32-bit vector index
  for (int64_t r0 = 0; r0 < rows; r0 += max_rows) {
    const int64_t nr = rows - r0 < max_rows ? rows - r0 : max_rows;
    launch(r0 * ld, (unsigned)(nr * cv), cv);
    MMF_CHECK_LAUNCH(fn);
  }
  return MMF_OK;
}

int bias_gelu_fwd(const char* fn, const void* x_bf16, const float* bias, void* y_bf16, int64_t rows, int cols, int ld, void* stream) {
  const unsigned short* x = static_cast<const unsigned short*>(x_bf16);
  unsigned short* y = static_cast<unsigned short*>(y_bf16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return bias_gelu_run(fn, x, y, y, bias, rows, cols, ld, [&](int64_t off, unsigned nvec, unsigned cv) {
    if (bias) hipLaunchKernelGGL(bias_gelu_kernel<true>, dim3(mmf_stream_grid(nvec, VIT_THREADS)), dim3(VIT_THREADS), 0, s, x + off, y + off, bias, nvec, cv, ld);
    else      hipLaunchKernelGGL(bias_gelu_kernel<false>, dim3(mmf_stream_grid(nvec, VIT_THREADS)), dim3(VIT_THREADS), 0, s, x + off, y + off, bias, nvec, cv, ld);
  });
}

}  // namespace

extern "C" int mmf_vit_patchify(const float* pixels, void* patches_bf16, int N, int C, int H, int W, int P, void* stream) {
  if (!pixels || !patches_bf16 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_vit_patchify: null operand or N=%d C=%d H=%d W=%d P=%d", N, C, H, W, P);
  if ((P & 7) || H % P || W % P)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_patchify: H=%d W=%d P=%d (needs P %% 8 == 0, H %% P == 0, W %% P == 0)", H, W, P);
  if (N > 65535) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_patchify: N=%d images in one call (at most 65535)", N);
  if (!mmf_aligned16(pixels) || !mmf_aligned16(patches_bf16))
    MMF_FAIL(MMF_E_ALIGN, "mmf_vit_patchify: pointers must be 16-byte aligned");
  const int64_t per_image = (int64_t)C * H * W / 8;                   // = gh * gw * C * P * P / 8 output vectors
  if (per_image >= (int64_t)1 << 31) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_patchify: image of %lld elements", (long long)per_image * 8);
  const unsigned kv = (unsigned)((int64_t)C * P * P / 8);
  hipLaunchKernelGGL(vit_patchify_kernel, dim3(mmf_stream_grid(per_image, VIT_THREADS), N), dim3(VIT_THREADS), 0, static_cast<hipStream_t>(stream),
                     pixels, static_cast<unsigned short*>(patches_bf16), C, H, W, P, W / P, kv, (unsigned)per_image);
  MMF_CHECK_LAUNCH("mmf_vit_patchify");
  return MMF_OK;
}

extern "C" int mmf_vit_embed_tokens(const void* patch_emb_bf16, const float* cls, const float* pos, void* tokens_bf16,
                                    int N, int T, int d, void* stream) {
  if (!patch_emb_bf16 || !cls || !pos || !tokens_bf16 || N <= 0 || T < 2 || d <= 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_vit_embed_tokens: null operand or N=%d T=%d d=%d", N, T, d);
  if (d & 7) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_embed_tokens: d=%d must be a multiple of 8", d);
  if (N > 65535 || (int64_t)T * d >= (int64_t)1 << 31)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_embed_tokens: N=%d (at most 65535), T*d=%lld (below 2^31)", N, (long long)T * d);
  if (!mmf_aligned16(patch_emb_bf16) || !mmf_aligned16(cls) || !mmf_aligned16(pos) || !mmf_aligned16(tokens_bf16))
    MMF_FAIL(MMF_E_ALIGN, "mmf_vit_embed_tokens: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(vit_embed_tokens_kernel, dim3(mmf_stream_grid((int64_t)T * d / 8, VIT_THREADS), N), dim3(VIT_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned short*>(patch_emb_bf16), cls, pos,
                     static_cast<unsigned short*>(tokens_bf16), T, d);
  MMF_CHECK_LAUNCH("mmf_vit_embed_tokens");
  return MMF_OK;
}

extern "C" int mmf_bias_gelu_bf16(void* x_bf16, const float* bias, int64_t rows, int cols, int ld, void* stream) {
  return bias_gelu_fwd("mmf_bias_gelu_bf16", x_bf16, bias, x_bf16, rows, cols, ld, stream);
}

extern "C" int mmf_bias_gelu_bf16_to(const void* h_bf16, const float* bias, void* g_bf16, int64_t rows, int cols, int ld, void* stream) {
  return bias_gelu_fwd("mmf_bias_gelu_bf16_to", h_bf16, bias, g_bf16, rows, cols, ld, stream);
}

extern "C" int mmf_bias_gelu_bwd_bf16(const void* dg_bf16, const void* h_bf16, const float* bias, void* dh_bf16, int64_t rows, int cols,
                                      int ld, void* stream) {
  const unsigned short *dg = static_cast<const unsigned short*>(dg_bf16), *h = static_cast<const unsigned short*>(h_bf16);
  unsigned short* dh = static_cast<unsigned short*>(dh_bf16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return bias_gelu_run("mmf_bias_gelu_bwd_bf16", dg, h, dh, bias, rows, cols, ld, [&](int64_t off, unsigned nvec, unsigned cv) {
    if (bias) hipLaunchKernelGGL(bias_gelu_bwd_kernel<true>, dim3(mmf_stream_grid(nvec, VIT_THREADS)), dim3(VIT_THREADS), 0, s, dg + off, h + off, bias, dh + off, nvec, cv, ld);
    else      hipLaunchKernelGGL(bias_gelu_bwd_kernel<false>, dim3(mmf_stream_grid(nvec, VIT_THREADS)), dim3(VIT_THREADS), 0, s, dg + off, h + off, bias, dh + off, nvec, cv, ld);
  });
}
