// The pieces a ViT forward has and the fusion path did not (mmfusion/vit.py): patch extraction for the patch-embedding
// GEMM, CLS / position tokens, exact GELU (gelu_erf of mmf_internal.h; and its backward, for the DeBERTa input gradient).  All are HBM-bound
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

// vit_embed_tokens_kernel's backward: a thread owns 8 columns of one token position t and walks the images in order, so
// dpos[t] (and dcls, for t = 0) += sum_n g[n][t] is one f32 chain per element in a fixed order with no atomics, and the rows
// t >= 1 are copied to the patch embedding's gradient on the way.  Four images' loads are in flight per thread (the rows of one
// position lie T * d elements apart); a wave reads 1 KiB contiguous per image.
__global__ __launch_bounds__(VIT_THREADS)
void vit_embed_tokens_bwd_kernel(const unsigned short* __restrict__ g, float* __restrict__ dcls, float* __restrict__ dpos,
                                 unsigned short* __restrict__ dpe, int N, int T, int d) {
  const unsigned dv = (unsigned)d >> 3, nvec = (unsigned)T * dv;
  const size_t img = (size_t)T * d, pimg = (size_t)(T - 1) * d;
  const unsigned stride = gridDim.x * VIT_THREADS;
  for (unsigned v = blockIdx.x * VIT_THREADS + threadIdx.x; v < nvec; v += stride) {
    const unsigned short* __restrict__ src = g + (size_t)v * 8;
    unsigned short* __restrict__ dst = v >= dv ? dpe + (size_t)(v - dv) * 8 : nullptr;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    int n = 0;
    for (; n + 4 <= N; n += 4) {
      u32x4_t w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const u32x4_t*>(src + (size_t)(n + u) * img);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[8];
        unpack8(w[u], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += f[e];
        if (dst) *reinterpret_cast<u32x4_t*>(dst + (size_t)(n + u) * pimg) = w[u];
      }
    }
    for (; n < N; ++n) {
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(src + (size_t)n * img);
      float f[8];
      unpack8(w, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += f[e];
      if (dst) *reinterpret_cast<u32x4_t*>(dst + (size_t)n * pimg) = w;
    }
    float* out = dpos + (size_t)v * 8;
    f32x4_t a = *reinterpret_cast<const f32x4_t*>(out), b = *reinterpret_cast<const f32x4_t*>(out + 4);
    *reinterpret_cast<f32x4_t*>(out) = a + f32x4_t{s[0], s[1], s[2], s[3]};
    *reinterpret_cast<f32x4_t*>(out + 4) = b + f32x4_t{s[4], s[5], s[6], s[7]};
    if (v < dv) {
      float* c = dcls + (size_t)v * 8;
      a = *reinterpret_cast<const f32x4_t*>(c), b = *reinterpret_cast<const f32x4_t*>(c + 4);
      *reinterpret_cast<f32x4_t*>(c) = a + f32x4_t{s[0], s[1], s[2], s[3]};
      *reinterpret_cast<f32x4_t*>(c + 4) = b + f32x4_t{s[4], s[5], s[6], s[7]};
    }
  }
}

// The attention backward of the CLS route's last layer: ONE query per image (row 0) over its T keys, on the fused q | k | v rows.
// A workgroup owns one (image, head): T dot products of DH each way, HBM-bound (k and v read twice, dk and dv written once), so it
// is plain f32 arithmetic and not the MFMA backward.  What it is for: mmf_attn_bwd_grouped takes delta = dO . O from the bf16 O,
// which leaves dO . (O - bf16(O)) as the sum of a row of dS; with one query that residue times the mean key is all of dq's error and
// it exceeded the storage model's at ViT-base sizes.  Here the softmax is formed again in f32 from the scores and
// delta = sum_j p_j dp_j, so a row of dS sums to zero up to f32 rounding.  LPK lanes share a key (8 columns each, the lanes past
// DH / 8 idle); every sum is reduced in a fixed order (lanes by butterfly, waves through LDS): two runs give the same bits.
constexpr int CLS_MAX_T = 4096;                                        // s and dp of every key live in LDS: 2 x 4 x T bytes
template <int DH>
__global__ __launch_bounds__(VIT_THREADS)
void vit_cls_attn_bwd_kernel(const unsigned short* __restrict__ qkv, const unsigned short* __restrict__ dout,
                             unsigned short* __restrict__ dqkv, int T, int d, float scale) {
  constexpr int LPK = DH == 64 ? 8 : 16, KPB = VIT_THREADS / LPK, NW = VIT_THREADS / 64;      // lanes per key, keys per pass, waves
  __shared__ float s_sc[CLS_MAX_T], s_dp[CLS_MAX_T];
  __shared__ float s_red[2][NW];
  __shared__ float s_dq[NW][DH];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, sub = tid % LPK, grp = tid / LPK;
  const bool live = sub * 8 < DH;
  const int ld = 3 * d;
  const size_t row0 = (size_t)b * T;
  const unsigned short* __restrict__ kbase = qkv + row0 * ld + d + h * DH + sub * 8;
  const unsigned short* __restrict__ vbase = kbase + d;
  float q[8], go[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { q[e] = 0.f; go[e] = 0.f; }
  if (live) {
    unpack8(*reinterpret_cast<const u32x4_t*>(qkv + row0 * ld + h * DH + sub * 8), q);
    unpack8(*reinterpret_cast<const u32x4_t*>(dout + (size_t)b * d + h * DH + sub * 8), go);
  }
  // pass 1: the scaled scores and dp_j = dO . v_j
  for (int j = grp; j < T; j += KPB) {
    float a = 0.f, c = 0.f;
    if (live) {
      float kv[8], vv[8];
      unpack8(*reinterpret_cast<const u32x4_t*>(kbase + (size_t)j * ld), kv);
      unpack8(*reinterpret_cast<const u32x4_t*>(vbase + (size_t)j * ld), vv);
#pragma unroll
      for (int e = 0; e < 8; ++e) { a += q[e] * kv[e]; c += go[e] * vv[e]; }
    }
#pragma unroll
    for (int o = LPK / 2; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
    if (sub == 0) { s_sc[j] = a * scale; s_dp[j] = c; }
  }
  __syncthreads();
  // the softmax over the T scores, and delta = sum_j p_j dp_j
  float m = -INFINITY;
  for (int j = tid; j < T; j += VIT_THREADS) m = fmaxf(m, s_sc[j]);
  m = wave_max(m);
  if ((tid & 63) == 0) s_red[0][tid >> 6] = m;
  __syncthreads();
  m = s_red[0][0];
#pragma unroll
  for (int w = 1; w < NW; ++w) m = fmaxf(m, s_red[0][w]);
  __syncthreads();
  float se = 0.f, sd = 0.f;
  for (int j = tid; j < T; j += VIT_THREADS) {
    const float e = expf(s_sc[j] - m);
    s_sc[j] = e;
    se += e;
    sd += e * s_dp[j];
  }
  se = wave_sum(se);
  sd = wave_sum(sd);
  if ((tid & 63) == 0) { s_red[0][tid >> 6] = se; s_red[1][tid >> 6] = sd; }
  __syncthreads();
  se = s_red[0][0];
  sd = s_red[1][0];
#pragma unroll
  for (int w = 1; w < NW; ++w) { se += s_red[0][w]; sd += s_red[1][w]; }
  const float inv = 1.f / se, delta = sd * inv;
  // pass 2: dS_j = p_j (dp_j - delta); dk_j = scale dS_j q, dv_j = p_j dO, dq = scale sum_j dS_j k_j
  float dq[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) dq[e] = 0.f;
  unsigned short* __restrict__ dkbase = dqkv + row0 * ld + d + h * DH + sub * 8;
  for (int j = grp; j < T; j += KPB) {
    if (live) {
      const float p = s_sc[j] * inv, ds = p * (s_dp[j] - delta), dss = ds * scale;
      float kv[8], ok[8], ov[8];
      unpack8(*reinterpret_cast<const u32x4_t*>(kbase + (size_t)j * ld), kv);
#pragma unroll
      for (int e = 0; e < 8; ++e) { dq[e] += ds * kv[e]; ok[e] = dss * q[e]; ov[e] = p * go[e]; }
      *reinterpret_cast<u32x4_t*>(dkbase + (size_t)j * ld) = pack8(ok);
      *reinterpret_cast<u32x4_t*>(dkbase + d + (size_t)j * ld) = pack8(ov);
    }
  }
  // dq: the key groups of a wave by butterfly (lanes LPK apart own the same columns), the waves through LDS
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int o = 32; o >= LPK; o >>= 1) dq[e] += __shfl_xor(dq[e], o, 64);
  if ((tid & 63) < LPK && live) {
#pragma unroll
    for (int e = 0; e < 8; ++e) s_dq[tid >> 6][sub * 8 + e] = dq[e];
  }
  __syncthreads();
  if (tid < LPK && live) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = s_dq[0][sub * 8 + e];
#pragma unroll
      for (int w = 1; w < NW; ++w) t += s_dq[w][sub * 8 + e];
      o[e] = t * scale;
    }
    *reinterpret_cast<u32x4_t*>(dqkv + row0 * ld + h * DH + sub * 8) = pack8(o);
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

// dh <- dg * gelu'(h + bias) (gelu_erf_grad of mmf_internal.h); dh may be dg.
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

// GELU with activation dropout (Wav2Vec2's intermediate_dropout), both directions in one kernel.  The rows are `items` items of
// `ipr` rows each; element (t, j) of item g is keyed by sub-stream item0 + g and index t * cols + j (MmfItemDrop, mmf_internal.h).
//   BWD false: y <- keep ? gelu(x + bias) c : 0, one rounding (x is the raw fc1 output and is left as it is unless y is x)
//   BWD true:  y <- keep ? dg c gelu'(x + bias) : 0, dg read from `dg` (y may be dg)
template <bool BWD>
__global__ __launch_bounds__(VIT_THREADS)
void bias_gelu_drop_kernel(const unsigned short* dg, const unsigned short* x, const float* __restrict__ bias, unsigned short* y, unsigned nvec,
                           unsigned cv /* cols/8 */, int ld, unsigned ipr, const MmfItemDrop dr) {
  const unsigned stride = gridDim.x * VIT_THREADS;
  const unsigned long long state = *dr.state;
  for (unsigned v = blockIdx.x * VIT_THREADS + threadIdx.x; v < nvec; v += stride) {
    const unsigned r = v / cv, j = (v - r * cv) << 3, g = r / ipr, t = r - g * ipr;
    const unsigned key = mmf_rng_key(state, dr.site, dr.item0 + g), idx = t * (cv << 3) + j;
    float a[8], d[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(x + (size_t)r * ld + j), a);
    if (BWD) unpack8(*reinterpret_cast<const u32x4_t*>(dg + (size_t)r * ld + j), d);
    const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(bias + j), b1 = *reinterpret_cast<const f32x4_t*>(bias + j + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xe = a[e] + (e < 4 ? b0[e] : b1[e - 4]);
      const bool keep = mmf_keep(key, idx + (unsigned)e, dr.thresh);
      const float val = BWD ? d[e] * dr.inv_keep * gelu_erf_grad(xe) : gelu_erf(xe) * dr.inv_keep;
      a[e] = keep ? val : 0.0f;
    }
    *reinterpret_cast<u32x4_t*>(y + (size_t)r * ld + j) = pack8(a);
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

extern "C" int mmf_vit_embed_tokens_bwd(const void* dtokens_bf16, float* dcls, float* dpos, void* dpatch_emb_bf16, int N, int T, int d,
                                        void* stream) {
  if (!dtokens_bf16 || !dcls || !dpos || !dpatch_emb_bf16 || N <= 0 || T < 2 || d <= 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_vit_embed_tokens_bwd: null operand or N=%d T=%d d=%d", N, T, d);
  if (d & 7) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_embed_tokens_bwd: d=%d must be a multiple of 8", d);
  if (N > 65535 || (int64_t)T * d >= (int64_t)1 << 31)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_embed_tokens_bwd: N=%d (at most 65535), T*d=%lld (below 2^31)", N, (long long)T * d);
  if (!mmf_aligned16(dtokens_bf16) || !mmf_aligned16(dcls) || !mmf_aligned16(dpos) || !mmf_aligned16(dpatch_emb_bf16))
    MMF_FAIL(MMF_E_ALIGN, "mmf_vit_embed_tokens_bwd: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(vit_embed_tokens_bwd_kernel, dim3(mmf_stream_grid((int64_t)T * d / 8, VIT_THREADS)), dim3(VIT_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned short*>(dtokens_bf16), dcls, dpos,
                     static_cast<unsigned short*>(dpatch_emb_bf16), N, T, d);
  MMF_CHECK_LAUNCH("mmf_vit_embed_tokens_bwd");
  return MMF_OK;
}

extern "C" int mmf_vit_cls_attn_bwd(const void* qkv_bf16, const void* dout_bf16, void* dqkv_bf16, int N, int H, int T, int head_dim,
                                    float scale, void* stream) {
  if (!qkv_bf16 || !dout_bf16 || !dqkv_bf16 || N <= 0 || H <= 0 || T <= 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_vit_cls_attn_bwd: null operand or N=%d H=%d T=%d", N, H, T);
  if (head_dim != 64 && head_dim != 96) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_cls_attn_bwd: head_dim=%d (supported: 64, 96)", head_dim);
  if (T > CLS_MAX_T || N > 65535 || H > 65535 || (int64_t)N * T * 3 * H * head_dim >= (int64_t)1 << 40)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_vit_cls_attn_bwd: T=%d (at most %d), N=%d, H=%d (at most 65535)", T, CLS_MAX_T, N, H);
  if (!mmf_aligned16(qkv_bf16) || !mmf_aligned16(dout_bf16) || !mmf_aligned16(dqkv_bf16))
    MMF_FAIL(MMF_E_ALIGN, "mmf_vit_cls_attn_bwd: pointers must be 16-byte aligned");
  const unsigned short *qkv = static_cast<const unsigned short*>(qkv_bf16), *dout = static_cast<const unsigned short*>(dout_bf16);
  unsigned short* dqkv = static_cast<unsigned short*>(dqkv_bf16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (head_dim == 64) hipLaunchKernelGGL(vit_cls_attn_bwd_kernel<64>, dim3(H, N), dim3(VIT_THREADS), 0, s, qkv, dout, dqkv, T, H * head_dim, scale);
  else                hipLaunchKernelGGL(vit_cls_attn_bwd_kernel<96>, dim3(H, N), dim3(VIT_THREADS), 0, s, qkv, dout, dqkv, T, H * head_dim, scale);
  MMF_CHECK_LAUNCH("mmf_vit_cls_attn_bwd");
  return MMF_OK;
}

extern "C" int mmf_bias_gelu_bf16(void* x_bf16, const float* bias, int64_t rows, int cols, int ld, void* stream) {
  return bias_gelu_fwd("mmf_bias_gelu_bf16", x_bf16, bias, x_bf16, rows, cols, ld, stream);
}

extern "C" int mmf_bias_gelu_bf16_to(const void* h_bf16, const float* bias, void* g_bf16, int64_t rows, int cols, int ld, void* stream) {
  return bias_gelu_fwd("mmf_bias_gelu_bf16_to", h_bf16, bias, g_bf16, rows, cols, ld, stream);
}

namespace {
// the two dropout entries: the plain entry's checks plus the items' geometry; a threshold of 0 takes the plain kernels
int bias_gelu_drop(const char* fn, bool bwd, const void* dg_bf16, const void* h_bf16, const float* bias, void* out_bf16, int64_t rows, int cols, int ld,
                   int64_t items, float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream) {
  MmfItemDrop dr;
  if (int rc = mmf_item_drop_fill(fn, p, rng_state, site, item0, &dr)) return rc;
  if (!bias) MMF_FAIL(MMF_E_SHAPE, "%s: null bias", fn);
  if (items <= 0 || rows <= 0 || rows % items) MMF_FAIL(MMF_E_SHAPE, "%s: rows=%lld are not items=%lld times a row count", fn, (long long)rows, (long long)items);
  if (cols <= 0 || (rows / items) * (int64_t)cols > ((int64_t)1 << 32) || rows * (int64_t)(cols >> 3) >= ((int64_t)1 << 31))
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: an item of %lld x %d elements (at most 2^32), %lld rows in all (rows * cols / 8 below 2^31)", fn,
             (long long)(rows / items), cols, (long long)rows);
  if (dr.thresh == 0u)
    return bwd ? mmf_bias_gelu_bwd_bf16(dg_bf16, h_bf16, bias, out_bf16, rows, cols, ld, stream)
               : mmf_bias_gelu_bf16_to(h_bf16, bias, out_bf16, rows, cols, ld, stream);
  const unsigned short *dg = static_cast<const unsigned short*>(dg_bf16), *h = static_cast<const unsigned short*>(h_bf16);
  unsigned short* out = static_cast<unsigned short*>(out_bf16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned ipr = (unsigned)(rows / items);
  return bias_gelu_run(fn, bwd ? dg : h, h, out, bias, rows, cols, ld, [&](int64_t off, unsigned nvec, unsigned cv) {      // (one piece: rows * cols / 8 < 2^31)
    if (bwd) hipLaunchKernelGGL(bias_gelu_drop_kernel<true>, dim3(mmf_stream_grid(nvec, VIT_THREADS)), dim3(VIT_THREADS), 0, s, dg + off, h + off, bias, out + off, nvec, cv, ld, ipr, dr);
    else     hipLaunchKernelGGL(bias_gelu_drop_kernel<false>, dim3(mmf_stream_grid(nvec, VIT_THREADS)), dim3(VIT_THREADS), 0, s, h + off, h + off, bias, out + off, nvec, cv, ld, ipr, dr);
  });
}
}  // namespace

extern "C" int mmf_bias_gelu_drop_bf16_to(const void* h_bf16, const float* bias, void* g_bf16, int64_t rows, int cols, int ld, int64_t items,
                                          float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream) {
  return bias_gelu_drop("mmf_bias_gelu_drop_bf16_to", false, nullptr, h_bf16, bias, g_bf16, rows, cols, ld, items, p, rng_state, site, item0, stream);
}

extern "C" int mmf_bias_gelu_drop_bwd_bf16(const void* dg_bf16, const void* h_bf16, const float* bias, void* dh_bf16, int64_t rows, int cols, int ld,
                                           int64_t items, float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream) {
  return bias_gelu_drop("mmf_bias_gelu_drop_bwd_bf16", true, dg_bf16, h_bf16, bias, dh_bf16, rows, cols, ld, items, p, rng_state, site, item0, stream);
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
