// What the three generations of the grouped bf16 GEMM (gemm2.hip, gemm6.hip, gemm7.hip) state once: the epilogue's element arithmetic,
// the tile order, the fill of the kernel-argument table and the "operand behind a buffer descriptor" rule.  Each keeps its own GemmArgs
// (the layouts differ by orig[], and kernel-argument offsets are scalar-load immediates); what they share is the fill, a template over both.
#pragma once
#include "mmf_internal.h"
#include <stddef.h>

namespace {

// ---- device: the epilogue of four consecutive outputs C[m][n .. n + 3] -------------------------------------------------------------
// The order of include/mmfusion.h (tests/keyed_dropout_ref.py restates it in float64) on the accumulators v (f32x4_t, changed in place;
// the bias is in them already where there is one):
//     ReLU -> dropout (mmf_keep of element IDX + e under key, kept values times scale) -> mask by the sign of aux -> alpha -> + aux.
// a: the four bf16 aux values as two packed words, read under MMF_EPI_MASK_AUX / MMF_EPI_ADD_AUX only.  IDX: m * N + n of v[0] (N, not ldc;
// mod 2^32), evaluated under the dropout flag only.  key: mmf_rng_key of the caller's problem index; scale: mmf_inv_keep(thresh).  Two forms:
//   MMF_EPI_QUAD_CT  flags at compile time (gemm6_parts.h's instantiated flag sets, gemm7.hip's drain).  The host sends these kernels
//                    alpha != 1 only with the mask (tile_epilogue, mmf_gemm7_supports): alpha rides on the mask's select;
//   MMF_EPI_QUAD_RT  flags at run time (gemm6_parts.h's general arm); do_drop is epi & MMF_EPI_DROPOUT, tested once by the caller.
//                    gemm2.hip's epilogue is this form with the aux load under a branch of its own and keeps its text (see there).
// Text, as MMF_G6_READ is, not function templates: through a function the dropout step came out in another instruction order in gemm7's
// dropout forms and all of gemm6 (index as argument or callable, threshold by value or reference: profiles/gemm_shared_parts.txt).
#define MMF_EPI_RELU4(v) _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) (v)[e_] = fmaxf((v)[e_], 0.f)
#define MMF_EPI_DROP4(v, IDX, key, thresh, scale)                                                                        \
  const unsigned idx_ = (IDX);                                                                                           \
  _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) (v)[e_] = mmf_keep(key, idx_ + e_, thresh) ? (v)[e_] * (scale) : 0.f
#define MMF_EPI_AUX4(a) const float a0_ = bf16lo((a)[0]), a1_ = bf16hi((a)[0]), a2_ = bf16lo((a)[1]), a3_ = bf16hi((a)[1])
#define MMF_EPI_QUAD_CT(CT_, v, a, IDX, key, thresh, scale, alpha)                                                       \
  do {                                                                                                                   \
    if constexpr ((CT_) & MMF_EPI_RELU) { MMF_EPI_RELU4(v); }                                                            \
    if constexpr ((CT_) & MMF_EPI_DROPOUT) { MMF_EPI_DROP4(v, IDX, key, thresh, scale); }                                \
    if constexpr ((CT_) & (MMF_EPI_MASK_AUX | MMF_EPI_ADD_AUX)) {                                                        \
      MMF_EPI_AUX4(a);                                                                                                   \
      if constexpr ((CT_) & MMF_EPI_MASK_AUX) {                                                                          \
        (v)[0] = a0_ > 0.f ? (v)[0] * (alpha) : 0.f; (v)[1] = a1_ > 0.f ? (v)[1] * (alpha) : 0.f;                        \
        (v)[2] = a2_ > 0.f ? (v)[2] * (alpha) : 0.f; (v)[3] = a3_ > 0.f ? (v)[3] * (alpha) : 0.f;                        \
      } else {                                                                                                           \
        (v)[0] += a0_; (v)[1] += a1_; (v)[2] += a2_; (v)[3] += a3_;                                                      \
      }                                                                                                                  \
    }                                                                                                                    \
  } while (0)
#define MMF_EPI_QUAD_RT(epi, do_drop, v, a, IDX, key, thresh, scale, alpha)                                              \
  do {                                                                                                                   \
    if ((epi) & MMF_EPI_RELU) { MMF_EPI_RELU4(v); }                                                                      \
    if (do_drop) { MMF_EPI_DROP4(v, IDX, key, thresh, scale); }                                                          \
    MMF_EPI_AUX4(a);                                                                                                     \
    if ((epi) & MMF_EPI_MASK_AUX) {                                                                                      \
      (v)[0] = a0_ > 0.f ? (v)[0] : 0.f; (v)[1] = a1_ > 0.f ? (v)[1] : 0.f;                                              \
      (v)[2] = a2_ > 0.f ? (v)[2] : 0.f; (v)[3] = a3_ > 0.f ? (v)[3] : 0.f;                                              \
    }                                                                                                                    \
    (v) *= (alpha);                                                                                                      \
    if ((epi) & MMF_EPI_ADD_AUX) { (v)[0] += a0_; (v)[1] += a1_; (v)[2] += a2_; (v)[3] += a3_; }                         \
  } while (0)

// ---- device: tile t of problem P -> (m0, n0), for tiles of TBM x TBN ---------------------------------------------------------------
// Super-rows of GROUP_M m-tiles, n fastest across a super-row: the ~32 tiles an XCD runs at the same time then form a GROUP_M x 4 block
// of the output and share A and B panels in that XCD's L2 (m fastest: 32 m-tiles of one n-tile, every A slice from the Infinity Cache).
template <int TBM, int TBN>
__device__ __forceinline__ void tile_origin(const mmf_gemm_problem& P, const int t, int& m0, int& n0) {
  const int tiles_m = (P.M + TBM - 1) / TBM, tiles_n = (P.N + TBN - 1) / TBN;
  // super-rows of 8 m-tiles.  (Round 4 tried the height that makes an XCD's 32 concurrent tiles touch the fewest operand panels — 32 / tiles_n
  // for narrow outputs, 11 x 3 instead of 8 x 3 + 8 x 1 at N = 768: the step got SLOWER, 2.027 -> 2.052 ms same box.)
  constexpr int GROUP_M = 8;
  const int grp = t / (GROUP_M * tiles_n), rem = t % (GROUP_M * tiles_n);
  const int gm = min(GROUP_M, tiles_m - grp * GROUP_M);
  m0 = (grp * GROUP_M + rem % gm) * TBM;
  n0 = (rem / gm) * TBN;
}

// ---- host: the kernel-argument table (either GemmArgs) -----------------------------------------------------------------------------
// Operands behind buffer descriptors (32-bit byte offsets) stay below 2 GiB: A and B in every generation, C and aux (or the bit buffer of
// MMF_EPI_RELU_BITS / MMF_EPI_MASK_BITS) in generation 7's drain as well (c_and_aux).
inline bool mmf_gemm_descriptors_fit(const mmf_gemm_problem& p, const int layout, const int epilogue, const bool c_and_aux) {
  constexpr size_t LIMIT = 0x7fffffffull;
  const size_t a_bytes = (size_t)(layout == MMF_GEMM_TN ? p.K : p.M) * p.lda * 2;
  const size_t b_bytes = (size_t)(layout == MMF_GEMM_NT ? p.N : p.K) * p.ldb * 2;
  if (a_bytes >= LIMIT || b_bytes >= LIMIT) return false;
  if (!c_and_aux) return true;
  const bool bits = (epilogue & (MMF_EPI_RELU_BITS | MMF_EPI_MASK_BITS)) != 0;
  const size_t c_bytes = (size_t)p.M * p.ldc * 2, x_bytes = bits ? mmf_gemm_relu_bits_bytes(p.M, p.N) : p.aux ? (size_t)p.M * p.ldaux * 2 : 0;
  return c_bytes < LIMIT && x_bytes < LIMIT;
}
// The head of a launch's table, no unit yet.  The dropout threshold travels only with its flag.
template <class Args>
void mmf_gemm_table_begin(Args& a, const int epilogue, const mmf_gemm_extra* extra) {
  a.nprob = 0;
  a.epi = epilogue;
  a.xcd_granule = mmf_xcd_granule();
  a.alpha = extra ? extra->alpha : 1.f;
  a.drop_thresh = (extra && (epilogue & MMF_EPI_DROPOUT)) ? mmf_drop_thresh(extra->dropout_p) : 0u;
  a.site = extra ? extra->site : 0u;
  a.rng_state = extra ? reinterpret_cast<const unsigned long long*>(extra->rng_state) : nullptr;
  a.tile_start[0] = 0;
}
// the next unit of the tile order (a problem; a chain of K segments) with its `tiles` tiles -> its index; a.tile_start[a.nprob]: tiles so far
template <class Args> int mmf_gemm_table_unit(Args& a, const int tiles) { a.tile_start[a.nprob + 1] = a.tile_start[a.nprob] + tiles; return a.nprob++; }
// the next problem as a unit of its own (which: the caller's index of it, for the message)
template <class Args>
int mmf_gemm_table_add(Args& a, const mmf_gemm_problem& p, const int tiles, const int which, const int layout, const bool c_and_aux) {
  if (!mmf_gemm_descriptors_fit(p, layout, a.epi, c_and_aux)) MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped[%d]: operand larger than 2 GiB", which);
  a.p[mmf_gemm_table_unit(a, tiles)] = p;
  return MMF_OK;
}
}  // namespace
