// Internal helpers shared by the gfx950 kernels of libmmfusion.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>
#include "../../include/mmfusion.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;   // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;

#define MMF_WAVE 64

// ---- error reporting (host) ---------------------------------------------------------------
void mmf_set_error(const char* fmt, ...);
#define MMF_FAIL(code, ...) do { mmf_set_error(__VA_ARGS__); return (code); } while (0)
#define MMF_CHECK_LAUNCH(name) do { hipError_t e_ = hipGetLastError(); \
  if (e_ != hipSuccess) MMF_FAIL(MMF_E_LAUNCH, "%s: launch failed: %s", name, hipGetErrorString(e_)); } while (0)

static inline bool mmf_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- bf16 <-> f32 (device) ------------------------------------------------------------------
// bf16 is carried as its 16-bit pattern.  f32 -> bf16 uses the plain cast so that hipcc emits
// v_cvt_pk_bf16_f32 (round-to-nearest-even, NaN stays NaN: MI355X_MICROARCH.md correctness table).
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
  return __uint_as_float(((unsigned)b) << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  typedef __attribute__((ext_vector_type(2))) float f32x2_t;
  f32x2_t v = {lo, hi};
  bf16x2_t h = __builtin_convertvector(v, bf16x2_t);
  return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ float bf16lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// eight bf16 (one 16-byte access) <-> eight f32: element 2 i is the low half of word i.  pack8 also takes the f32 side as two halves.
__device__ __forceinline__ void unpack8(const u32x4_t& w, float (&f)[8]) {
  f[0] = bf16lo(w[0]); f[1] = bf16hi(w[0]); f[2] = bf16lo(w[1]); f[3] = bf16hi(w[1]);
  f[4] = bf16lo(w[2]); f[5] = bf16hi(w[2]); f[6] = bf16lo(w[3]); f[7] = bf16hi(w[3]);
}
__device__ __forceinline__ u32x4_t pack8(const float (&f)[8]) {
  return u32x4_t{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                 pack_bf16x2(f[6], f[7])};
}
__device__ __forceinline__ u32x4_t pack8(const f32x4_t a, const f32x4_t b) {
  return u32x4_t{pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]), pack_bf16x2(b[2], b[3])};
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// The exact GELU, the project's only forward: gelu(x) = x Phi(x) with Phi(x) = erfc(|x| / sqrt 2) / 2 for x < 0 and 1 - that otherwise.
// 1 + erf(x / sqrt 2) rounds away every digit of Phi in the left tail (x = -5: 20 bf16 ulps of the result, an exact -0 from x = -5.44
// down), and FFN pre-activations and a normalisation's output both reach it, so the kernels' outputs would not be within a bf16 ulp of
// the exact value.  erfc(z), z >= 0, is the Chebyshev fit t exp(-z^2 + P(t)), t = 1 / (1 + z / 2) (Numerical Recipes' erfcc: a RELATIVE
// error near 1e-7 for every z; in f32 with v_rcp and v_exp the GELU stays within 2e-5 of its value until Phi itself falls under the
// smallest normal f32 near x = -13), a third of erfcf's instructions: the layer-norm family's two kernels are near their ALU bound beside
// the memory one.  tests/gelu_domain.py holds every site to float64 over all finite bf16 inputs.
__device__ __forceinline__ float gelu_erf(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f, t = __builtin_amdgcn_rcpf(fmaf(0.5f, z, 1.0f));
  float p = 0.17087277f;
  p = fmaf(p, t, -0.82215223f);
  p = fmaf(p, t, 1.48851587f);
  p = fmaf(p, t, -1.13520398f);
  p = fmaf(p, t, 0.27886807f);
  p = fmaf(p, t, -0.18628806f);
  p = fmaf(p, t, 0.09678418f);
  p = fmaf(p, t, 0.37409196f);
  p = fmaf(p, t, 1.00002368f);
  p = fmaf(p, t, -1.26551223f);
  const float h = 0.5f * t * __expf(fmaf(-z, z, p));                  // Phi(-|x|)
  return x * (x < 0.0f ? h : 1.0f - h);
}
// gelu'(v) = Phi(v) + v phi(v).  Phi through erfc: 1 + erf(v / sqrt 2) loses every digit of Phi in the left tail (v < -5), where
// v phi(v) is just as small and the derivative would be f32 noise.
__device__ __forceinline__ float gelu_erf_grad(float v) {
  return 0.5f * erfcf(v * -0.70710678118654752440f) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

// ---- streaming launches -----------------------------------------------------------------------
// Grid of a grid-stride streaming kernel over nvec per-lane accesses: one workgroup per `threads` of them, 1 .. 2048
// (cdna_hip_programming.md Guideline 11/13: enough workgroups to fill the chip, the loop takes the rest).
static inline int mmf_stream_grid(int64_t nvec, int threads) {
  int64_t g = (nvec + threads - 1) / threads;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}
// Grouped launch: problem i owns workgroups [blk_start[i], blk_start[i + 1]) and blk_start[n] is the grid.  The problem
// of workgroup `bid`, wave-uniform (n is a few dozen at most and blk_start sits in the kernel arguments: a scalar scan).
template <int N>
__device__ __forceinline__ int mmf_group_problem(const int (&blk_start)[N], int n, int bid) {
  int pi = 0;
  while (pi + 1 < n && bid >= blk_start[pi + 1]) ++pi;
  return pi;
}

// ---- wave reductions ------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- tile id of workgroup `orig` in a grouped launch of `total` tiles -----------------------------------
// The dispatcher deals workgroups to the 8 XCDs round-robin (orig % 8) and in order, so XCD x runs ids x, x+8, ...
// Tiles are handed out in GRANULES of G consecutive tile ids, granule g to XCD g % 8: the tiles an XCD runs at
// one time are still neighbours (they share A/B panels in that XCD's L2), and every XCD gets the same mix of
// problems.  One contiguous range per XCD (G = 0, the first form) is only balanced when all tiles take equally
// long: with the problems ordered by K descending it gave XCD 0 nothing but the longest tiles and the launch
// ended when XCD 0 did.  The last (< 8 G) tiles, and launches smaller than that, keep one range per XCD.
__host__ __device__ __forceinline__ int mmf_xcd_tile(int orig, int total, int G) {   // (host: gemm7.hip's tile-width choice)
  const int xcd = orig & 7;
  const int full = G > 0 ? (total / (8 * G)) * (8 * G) : 0;
  if (orig < full) {
    const int j = orig >> 3;
    return ((j / G) * 8 + xcd) * G + (j % G);
  }
  const int rest = total - full, q = rest >> 3, r = rest & 7;
  return full + (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + ((orig - full) >> 3);
}
static inline int mmf_xcd_granule() {                       // host: MMF_GEMM_XCD_GRANULE (default 32, 0 = first form)
  static const int g = [] { const char* e = getenv("MMF_GEMM_XCD_GRANULE"); const int v = e ? atoi(e) : 32; return v > 0 ? v : 0; }();
  return g;
}

// ---- counter-based dropout RNG -----------------------------------------------------------------------
// keep(e) for element e of dropout call-site `site`, stream `sub` (problem / (b,h) index) under the
// DEVICE-resident 64-bit state `seed`: two rounds of the lowbias32 integer hash.  Stateless, so the
// backward pass regenerates the forward's mask instead of storing it, and because the state lives in
// device memory (advanced once per training step by the host side) a replayed hipGraph draws fresh
// masks every step.  keep probability = 1 - p with p quantised to 2^-32.
__device__ __forceinline__ unsigned mmf_mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ unsigned mmf_rng_key(unsigned long long seed, unsigned site, unsigned sub) {
  return mmf_mix32((unsigned)seed ^ (site * 0x9E3779B9u)) ^ (unsigned)(seed >> 32) ^ (sub * 0x85EBCA6Bu);
}
__device__ __forceinline__ bool mmf_keep(unsigned key, unsigned idx, unsigned thresh) {
  return mmf_mix32(key + idx * 0x9E3779B9u) >= thresh;
}
static inline unsigned mmf_drop_thresh(float p) {          // host: p in [0, 1)
  double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}
// what a kept value is multiplied by: 1 / (1 - p) with p as mmf_drop_thresh quantised it.  thresh == 0 (no dropout) gives 1.f by the
// arithmetic itself (1 / (1 - 0)), so there is no branch on it: the GEMM epilogues call this under their own DROP guard and keep
// the instructions they had.  The host restatements (tests/attn_ref.py: inv_keep_of) form the same f32 operations in this order
__host__ __device__ __forceinline__ float mmf_inv_keep(unsigned thresh) {
  return 1.f / (1.f - (float)thresh * (1.f / 4294967296.f));
}
// What a kernel with keyed dropout takes by value (hidden dropout in elementwise.hip, the Wav2Vec2 regularisers of vit.hip / wav2vec2.hip,
// DeBERTa's attention in deberta.hip, the delta pre-pass of attention.hip): element e of item g is
// mmf_keep(mmf_rng_key(*state, site, item0 + g), e, thresh), kept values are multiplied by inv_keep.  The attention kernels key a (item,
// head) pair: DeBERTa's sub-stream is (item0 + item) H + h, the delta pre-pass takes its stream base in item0 (sub-stream item0 + b H + h)
struct MmfItemDrop {
  const unsigned long long* state;                             // the device-resident 64-bit RNG state
  unsigned site, thresh, item0;                                // the sub-stream is a 32-bit value: item0 + item wraps as the hash's input does
  float inv_keep;                                              // mmf_inv_keep(thresh)
};
// host: the checks the entries with (p, rng_state, site, item0) share -> dr.  thresh == 0 (p = 0 or below 2^-32): no dropout, state may
// be NULL (an entry with a plain kernel form then takes it)
static inline int mmf_item_drop_fill(const char* fn, float p, const uint64_t* rng_state, uint32_t site, int64_t item0, MmfItemDrop* dr) {
  if (!(p >= 0.0f) || p >= 1.0f) MMF_FAIL(MMF_E_SHAPE, "%s: p=%g outside [0, 1)", fn, (double)p);
  if (item0 < 0) MMF_FAIL(MMF_E_SHAPE, "%s: item0=%lld is negative", fn, (long long)item0);
  const unsigned thresh = mmf_drop_thresh(p);
  if (thresh != 0u && !rng_state) MMF_FAIL(MMF_E_SHAPE, "%s: null rng_state with p=%g", fn, (double)p);
  if (reinterpret_cast<uintptr_t>(rng_state) & 7u) MMF_FAIL(MMF_E_ALIGN, "%s: rng_state must be 8-byte aligned", fn);
  dr->state = reinterpret_cast<const unsigned long long*>(rng_state);
  dr->site = site;
  dr->thresh = thresh;
  dr->item0 = (unsigned)item0;
  dr->inv_keep = mmf_inv_keep(thresh);
  return MMF_OK;
}

// transposed LDS read (ds_read_b64_tr_b16): per 16-lane group a 4-row x 16-column block of
// 16-bit elements; lane 4q+p supplies the address of row q, columns 4p..4p+3; lane i receives
// column i of the four rows (cdna_hip_programming.md T10).  EXEC must be all ones.
__device__ __forceinline__ s16x4_t lds_read_tr16(const void* lds_addr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4_t*)(lds_addr));
}
