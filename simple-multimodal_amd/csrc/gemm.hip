// Grouped bf16 GEMM on the gfx950 matrix cores (v_mfma_f32_16x16x32_bf16 in gemm2, v_mfma_f32_32x32x16_bf16 in gemm6 / gemm7), f32
// accumulate: C-ABI entry points, validation and the choice of kernel generation.
//
// One launch = up to MMF_GEMM_MAX_PROBLEMS independent problems (the six cross-modal blocks'
// projections / FFNs of MulT, models/fusion_layers.py:146-153, are issued together so the grid
// has >> 256 workgroups even though each problem is small).  The problem table travels by value
// in the kernel arguments, so a launch is self-contained and hipGraph-capturable.
//
// Kernels (three): gemm2.hip (LDS-DMA ring, 256 x 128 tile, eight waves: the general kernel — any K, small launches),
// gemm6.hip (256 x 256 tile, one wave per SIMD with 128 x 128 wave tiles, a 32-deep x 4-stage LDS ring, one tile per workgroup: wgrad,
// and every NT / NN launch the persistent form refuses — f32 output, a flag set it does not instantiate, alpha != 1 anywhere but on the
// NN ReLU mask, K < 160, N or a leading dimension of C / aux no multiple of 8, an aux that is not 16-byte aligned) and gemm7.hip (gemm6's
// tile and ring walked by persistent workgroups, outputs through LDS: every NT / NN launch it takes once the automatic choice below has given
// the launch generation 6); gemm6_parts.h holds what the last two share, gemm_common.h what all three do (epilogue arithmetic, tile order,
// table fill).  Without a bias generation 7 is bit-identical to generation 6; with one a small fraction of the outputs differ by one bf16 ulp.
// Earlier generations — the register-staged 128 x 128 kernel and gemm3 (rounds 1-2), gemm4 (256 x 256 ring, eight waves; stream-K) and gemm5 (32-deep ring, two workgroups per CU)
// (rounds 2-3) — are in git history with their measurements in DESIGN.md section 5; the last two left in round 4, when a same-box
// A/B of the selection rule without them came out level or ahead on all four workloads (MulT 2.116 -> 2.088 ms, hierarchical
// 2.75 = 2.75, training step 3.33 -> 3.34, MELD-shaped 1.076 -> 1.070).
#include "mmf_internal.h"
#include <stdlib.h>

int mmf_gemm2_launch(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue,
                     int out_f32, const mmf_gemm_extra* extra, hipStream_t s);   // gemm2.hip: LDS-DMA ring kernel
int mmf_gemm6_launch(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue,
                     int out_f32, const mmf_gemm_extra* extra, hipStream_t s);   // gemm6.hip: one wave per SIMD, 128x128 wave tiles
bool mmf_gemm6_supports(const mmf_gemm_problem* problems, int num_problems, int layout);
bool mmf_gemm6_supports_epi(int epilogue, int out_f32);
int mmf_gemm7_launch(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue,
                     int out_f32, const mmf_gemm_extra* extra, hipStream_t s);   // gemm7.hip: gemm6's tile, persistent workgroups
bool mmf_gemm7_supports(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue, int out_f32, const mmf_gemm_extra* extra);

// Implementation switch (A/B runs in one process: tools/gemm7_bench.py): 0 = automatic (default), 2 / 6 / 7 = that kernel for every
// launch it supports.  Default from MMF_GEMM_IMPL, else automatic.
static bool impl_built(int v) { return v == 0 || v == 2 || v == 6 || v == 7; }
static int g_gemm_impl = [] {
  const char* e = getenv("MMF_GEMM_IMPL");
  const int v = (e && e[0] >= '0' && e[0] <= '9') ? e[0] - '0' : 0;
  return impl_built(v) ? v : 0;
}();

// The automatic choice: the 256 x 256 one-wave-per-SIMD tile for every launch it supports that gives at least a quarter of the CUs a
// tile (wgrad: half — a single layer's weight gradient keeps the 256 x 128 ring and its twice as many tiles), gemm2 for the rest.
static int auto_impl(const mmf_gemm_problem* p, int n, int layout) {
  long tiles = 0;
  for (int i = 0; i < n; ++i) tiles += (long)((p[i].M + 255) / 256) * ((p[i].N + 255) / 256);
  static const int cus = [] { int c = mmf_device_cu_count(); return c > 0 ? c : 256; }();
  const long need = layout == MMF_GEMM_TN ? (cus + 1) / 2 : (cus + 3) / 4;
  return (tiles >= need && mmf_gemm6_supports(p, n, layout)) ? 6 : 2;
}
static int gemm_impl() { return g_gemm_impl; }
static thread_local int t_last_impl = 0;
extern "C" int mmf_gemm_last_impl(void) { return t_last_impl; }
extern "C" int mmf_gemm_select_impl(int impl) {
  if (!impl_built(impl))
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_select_impl: generation %d is not built (0 = automatic, 2, 6, 7; 1 / 3 left in round 3, 4 / 5 in round 4)", impl);
  g_gemm_impl = impl;
  return MMF_OK;
}

// the kernel generation a launch goes to: the pinned or automatic choice, falling back 7 -> 6 -> 2 to one that takes it
static int select_impl(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue, int out_f32, const mmf_gemm_extra* extra) {
  int impl = gemm_impl();
  const bool pinned = impl != 0;
  if (impl == 0) impl = auto_impl(problems, num_problems, layout);
  const bool ok6 = mmf_gemm6_supports(problems, num_problems, layout) && mmf_gemm6_supports_epi(epilogue, out_f32);
  if (impl == 6 && !pinned && mmf_gemm7_supports(problems, num_problems, layout, epilogue, out_f32, extra)) impl = 7;
  if (impl == 7 && !mmf_gemm7_supports(problems, num_problems, layout, epilogue, out_f32, extra)) impl = 6;
  if (impl == 6 && !ok6) impl = 2;
  return impl;
}

constexpr int EPI_BITS = MMF_EPI_RELU_BITS | MMF_EPI_MASK_BITS;
// the flag combinations the bit forms allow (whether generation 7 instantiates the set is mmf_gemm7_supports's answer)
static bool bits_flags_ok(int epilogue) {
  if ((epilogue & EPI_BITS) == EPI_BITS || (epilogue & (MMF_EPI_MASK_AUX | MMF_EPI_ADD_AUX))) return false;   // one owner of aux
  return (epilogue & MMF_EPI_RELU_BITS) ? (epilogue & MMF_EPI_RELU) != 0 : true;
}

// What the entry points ask of ONE problem, whichever generation takes the launch -> MMF_OK, or the code with the reason in `why`
// (nullptr: only ask).  mmf_gemm_grouped_ex asks it per problem, the chain form (gemm7.hip) per segment.
int mmf_gemm_problem_fault(const mmf_gemm_problem& p, int layout, int epilogue, char* why, size_t why_bytes) {
#define MMF_FAULT(code, ...) do { if (why) snprintf(why, why_bytes, __VA_ARGS__); return (code); } while (0)
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) MMF_FAULT(MMF_E_SHAPE, "empty problem M=%d N=%d K=%d", p.M, p.N, p.K);
  if (!p.A || !p.B || !p.C) MMF_FAULT(MMF_E_SHAPE, "null operand");
  if ((epilogue & (MMF_EPI_BIAS | MMF_EPI_COLSUM_A)) && !p.bias) MMF_FAULT(MMF_E_SHAPE, "bias is null");
  if ((epilogue & (MMF_EPI_MASK_AUX | MMF_EPI_ADD_AUX | EPI_BITS)) && !p.aux) MMF_FAULT(MMF_E_SHAPE, "aux is null");
  // the contiguous extent of each operand must be a multiple of 8 elements (16-B vector loads)
  const int a_cols = (layout == MMF_GEMM_TN) ? p.M : p.K;
  const int b_cols = (layout == MMF_GEMM_NT) ? p.K : p.N;
  if ((a_cols & 7) || (b_cols & 7) || (p.lda & 7) || (p.ldb & 7) || (p.N & 3) || (p.ldc & 3) ||
      ((epilogue & (MMF_EPI_MASK_AUX | MMF_EPI_ADD_AUX)) && (p.ldaux & 3)))
    MMF_FAULT(MMF_E_ALIGN, "M=%d N=%d K=%d lda=%d ldb=%d ldc=%d ldaux=%d violate the 8-element (operands) / 4-element (output) granularity",
              p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.ldaux);
  if (p.lda < a_cols || p.ldb < b_cols || p.ldc < p.N) MMF_FAULT(MMF_E_SHAPE, "leading dimension smaller than the row");
  // (aux at 8 bytes: generations 2 and 6 read it in 8-byte pieces; generation 7 asks for 16, mmf_gemm7_supports)
  if (!mmf_aligned16(p.A) || !mmf_aligned16(p.B) || !mmf_aligned16(p.C) ||
      (p.bias && !mmf_aligned16(p.bias)) || (p.aux && (reinterpret_cast<uintptr_t>(p.aux) & 7)))
    MMF_FAULT(MMF_E_ALIGN, "operand pointers must be 16-byte aligned");
#undef MMF_FAULT
  return MMF_OK;
}

extern "C" size_t mmf_gemm_relu_bits_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)((M + 31) / 32) * (size_t)((N + 31) / 32) * 64 * sizeof(uint16_t);
}

extern "C" int mmf_gemm_relu_bits_available(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue,
                                            int out_f32, const mmf_gemm_extra* extra) {
  if (!problems || num_problems <= 0 || num_problems > MMF_GEMM_MAX_PROBLEMS || !(epilogue & EPI_BITS) || !bits_flags_ok(epilogue)) return 0;
  return select_impl(problems, num_problems, layout, epilogue, out_f32, extra) == 7;
}

extern "C" int mmf_gemm_grouped(const mmf_gemm_problem* problems, int num_problems, int layout,
                                int epilogue, int out_f32, void* stream) {
  return mmf_gemm_grouped_ex(problems, num_problems, layout, epilogue, out_f32, nullptr, stream);
}

extern "C" int mmf_gemm_grouped_ex(const mmf_gemm_problem* problems, int num_problems, int layout,
                                   int epilogue, int out_f32, const mmf_gemm_extra* extra, void* stream) {
  if (!problems || num_problems <= 0 || num_problems > MMF_GEMM_MAX_PROBLEMS)
    MMF_FAIL(MMF_E_SHAPE, "mmf_gemm_grouped: num_problems=%d out of range [1,%d]", num_problems,
             MMF_GEMM_MAX_PROBLEMS);
  if (layout < MMF_GEMM_NT || layout > MMF_GEMM_TN)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: unknown layout %d", layout);
  if ((epilogue & MMF_EPI_ACCUM) && !out_f32)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: MMF_EPI_ACCUM needs f32 output");
  if ((epilogue & MMF_EPI_MASK_AUX) && (epilogue & MMF_EPI_ADD_AUX))
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: MASK_AUX and ADD_AUX are exclusive");
  if ((epilogue & MMF_EPI_COLSUM_A) && (layout != MMF_GEMM_TN || (epilogue & MMF_EPI_BIAS)))
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: COLSUM_A is a TN (wgrad) epilogue and excludes BIAS");
  if ((epilogue & EPI_BITS) && !bits_flags_ok(epilogue))
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: RELU_BITS needs RELU; RELU_BITS, MASK_BITS, MASK_AUX and ADD_AUX are exclusive (one aux pointer)");
  if (epilogue & MMF_EPI_DROPOUT) {
    if (!extra || !extra->rng_state || !(extra->dropout_p >= 0.f) || extra->dropout_p >= 1.f)
      MMF_FAIL(MMF_E_SHAPE, "mmf_gemm_grouped_ex: MMF_EPI_DROPOUT needs rng_state and 0 <= p < 1");
  }
  const int impl = select_impl(problems, num_problems, layout, epilogue, out_f32, extra);
  if ((epilogue & EPI_BITS) && impl != 7)
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: RELU_BITS / MASK_BITS exist in generation 7 only and this launch goes to generation %d "
             "(mmf_gemm_relu_bits_available)", impl);
  t_last_impl = impl;
  char why[256];
  for (int i = 0; i < num_problems; ++i)
    if (const int e = mmf_gemm_problem_fault(problems[i], layout, epilogue, why, sizeof why)) MMF_FAIL(e, "mmf_gemm_grouped[%d]: %s", i, why);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (impl == 2) return mmf_gemm2_launch(problems, num_problems, layout, epilogue, out_f32, extra, s);
  if (impl == 6) return mmf_gemm6_launch(problems, num_problems, layout, epilogue, out_f32, extra, s);
  if (impl == 7) return mmf_gemm7_launch(problems, num_problems, layout, epilogue, out_f32, extra, s);
  MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: kernel generation %d is not built (2, 6, 7)", impl);
}

// ---- K-segment chains: C = sum over a chain's segments of A_s B_s, one accumulator chain per output tile (gemm7.hip) -----------------
bool mmf_gemm7_chain_supports(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue);
int mmf_gemm7_chain_launch(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue, hipStream_t s);

// generation 7 only: a pinned generation 2 or 6 (mmf_gemm_select_impl) has no chain form
extern "C" int mmf_gemm_chain_available(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue, void* /*stream*/) {
  return (gemm_impl() == 0 || gemm_impl() == 7) && mmf_gemm7_chain_supports(chains, num_chains, layout, epilogue);
}

extern "C" int mmf_gemm_grouped_chain(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue, void* stream) {
  if (!mmf_gemm_chain_available(chains, num_chains, layout, epilogue, stream))
    MMF_FAIL(MMF_E_SHAPE, "mmf_gemm_grouped_chain: %d chains, layout %d, epilogue %d: not a launch of the chain form (NN, bf16 output, flags none / "
             "MMF_EPI_BIAS / MMF_EPI_ADD_AUX, 1..%d segments of K %% 32 == 0 and K >= 160, generation 7 selectable; mmf_gemm_chain_available)",
             num_chains, layout, epilogue, MMF_GEMM_CHAIN_MAX_SEGMENTS);
  t_last_impl = 7;
  return mmf_gemm7_chain_launch(chains, num_chains, layout, epilogue, static_cast<hipStream_t>(stream));
}
