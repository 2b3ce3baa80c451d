// Grouped bf16 GEMM, PERSISTENT one-wave-per-SIMD form (round 4): the 256 x 256 tile / 128 x 128 wave-tile kernel of gemm6.hip with
// one workgroup per CU walking a list of tiles, its LDS ring running on ACROSS tile boundaries.
//
// Why.  A K = 768 tile of gemm6 is 2.7 us of prologue (the ring fill: 128 KiB per CU requested by all 256 CUs at once), 15.4 us of
// k-loop and 4-5 us of epilogue, and in a launch of one to three rounds every CU is in the same phase at the same time: the
// prologue is an HBM burst with the matrix pipe idle, the epilogue a store burst (rounds 2-3; measured with
// gemm6's no-epilogue ablation build, in git history as of the parent of the commit that removed the ablation builds).  Here
//   * workgroup w (one per CU, grid = min(tiles, CUs)) takes the tiles w, w + grid, ... of the launch's XCD-aware tile order
//     (mmf_xcd_tile: an XCD's 32 workgroups still share A / B panels in its L2);
//   * the LDS-DMA stream never stops: while tile j's last NS stages are multiplied, the refills of the ring fetch the first NS
//     stages of tile j + 1 (descriptors and per-lane source offsets switch at the hand-over of stage KT - NS), so tile j + 1's
//     first fragments are read behind the last MFMAs of tile j — no ring fill except the workgroup's very first;
//   * a tile's outputs are stored between its last stage and the next tile's first; the stores are not waited for (the stage
//     hand-overs keep their piece-only vmcnt counts: with stores in flight they wait for MORE than they need, never for less —
//     vmcnt counts loads and stores together) and drain under the next tile's k-loop.
// NT and NN, bf16 output, every K a multiple of 32 and >= (NS + 1) * 32; everything else stays on gemm6 (gemm.hip).
//
// Two tile widths (TN: n-fragments per wave).  TN = 4 is gemm6's 256 x 256 tile (wave tile 128 x 128); TN = 3 a 256 x 192 tile (wave
// tile 128 x 96).  Every N of the fusion step is a multiple of 768 = 3 x 256 = 4 x 192, and a launch of 354 tiles on 256 CUs ends on a
// round of 98 tiles with 158 CUs idle; at 192 the same launch is 472 tiles of three quarters the work.  The host (pick_tile_n) takes
// the narrower form only where the walk's makespan is strictly shorter.  Both forms give every output element the same MFMA chain
// (bias start, then the k-substeps in order) and no K split: the results are bit-identical.
#include <algorithm>
#include <vector>
#include "gemm6_parts.h"

namespace {

constexpr int TILE = 256 * BK * 2, PPO = BK / 8;             // the m-operand tile: 16 KiB, 4 pieces per wave and stage
// the n-operand tile of the TN form: TN * 64 columns, TN * 4 KiB (TN pieces per wave); a stage holds both tiles
template <int TN> struct Form {
  static constexpr int BNT = 64 * TN, TILE_B = BNT * BK * 2, STAGE = TILE + TILE_B, PPB = TN, PPW = PPO + PPB;
  static constexpr int LDS = NS * STAGE + 4 * 8192;          // the ring and the four waves' output staging regions
};
static_assert(Form<4>::LDS == 160 * 1024 && Form<3>::LDS == 144 * 1024, "LDS of the two forms");

// what the fetch side needs of the NEXT tile (wave-uniform): first element of each operand tile, bytes from there to the operand's
// last valid element (< 2 GiB: host), bytes per stage of the n-operand, stages
struct TileSrc {
  const unsigned short* Ab;
  const unsigned short* Bb;
  int recA, recB, stepB, KT;
};
// what the compute / store side needs (last: a chain launch's entry is its tile's last K segment, the one that is drained)
struct TileDst {
  int pi, m0, n0;
  bool last;
};

// A wave-uniform value the vector ALU produced (integer division has no scalar form), handed to the scalar side.  As an inline-asm
// statement on purpose: the builtin is folded away wherever the compiler can prove its operand uniform, and the loop-carried
// descriptor chain that depends on it then lands in VECTOR registers — the "s" operands of the LDS-DMA statements print as VGPR
// quads and the assembler rejects them (seen with this kernel's tile loop; gemm6 has no such loop).
__device__ __forceinline__ int to_sgpr(int x) {
  int r;
  // wait states INSIDE the string (hipcc pads nothing around an asm statement): one between a vector write of x and the
  // readfirstlane (without it m0 / n0 came back stale: a memory fault on the first launch), five before a memory instruction may
  // read the scalar the vector ALU wrote
  asm volatile("s_nop 0\n\tv_readfirstlane_b32 %0, %1\n\ts_nop 4" : "=s"(r) : "v"(x));
  return r;
}

// CHAIN: the launch's units are chains of K segments (GemmArgs::orig); the entry is segment `seg` of tile `orig` of the chains'
// tile order.  A chain's segments are problems of one M, N and C, so the tile's origin and its output side are any segment's.
template <bool B_KR, int TN, bool CHAIN>
__device__ __forceinline__ void locate_tile(const GemmArgs& args, const int total_tiles, const int orig, const int seg, TileSrc& s, TileDst& d, int& lda, int& ldb) {
  const int bid = to_sgpr(mmf_xcd_tile(orig, total_tiles, args.xcd_granule));
  int pi = 0;
  while (pi + 1 < args.nprob && bid >= args.tile_start[pi + 1]) ++pi;
  const int t = bid - args.tile_start[pi];
  d.last = true;
  if constexpr (CHAIN) {
    d.last = args.orig[pi] + seg + 1 == args.orig[pi + 1];
    pi = args.orig[pi] + seg;
  }
  const mmf_gemm_problem& P = args.p[pi];
  int m0, n0;
  tile_origin<BM, Form<TN>::BNT>(P, t, m0, n0);
  m0 = to_sgpr(m0);
  n0 = to_sgpr(n0);
  d.pi = pi; d.m0 = m0; d.n0 = n0;
  lda = P.lda; ldb = P.ldb;
  s.Ab = static_cast<const unsigned short*>(P.A) + (size_t)m0 * P.lda;
  s.Bb = static_cast<const unsigned short*>(P.B) + (B_KR ? (size_t)n0 : (size_t)n0 * P.ldb);
  s.recA = (int)(((long)(P.M - m0 - 1) * P.lda + P.K) * 2);
  s.recB = (int)((B_KR ? ((long)(P.K - 1) * P.ldb + (P.N - n0)) : ((long)(P.N - n0 - 1) * P.ldb + P.K)) * 2);
  s.stepB = (B_KR ? BK * P.ldb : BK) * 2;
  s.KT = P.K / BK;
}

// ---- the ReLU / dropout keep-mask as bits (drain_tile: MMF_EPI_RELU_BITS writes them, MMF_EPI_MASK_BITS applies them) ---------------
// NOT (x > 0) of the two bf16 halves of w, 0 / 1 per half, in three packed 16-bit operations: as a bit pattern x > 0 is
// 1 <= x <= 0x7f80 (+inf), that is x - 1 (wrapping: 0 -> 0xffff) < 0x7f80, that is bit 15 of the saturating (x - 1) + 0x80 clear.
// Exact for every pattern (zeros, negatives and NaNs of either sign are not positive), as bf16lo(w) > 0.f is.
__device__ __forceinline__ unsigned bf16x2_not_positive(unsigned w) {
  typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
  const u16x2_t y = __builtin_bit_cast(u16x2_t, w) - (u16x2_t){1, 1};
  const u16x2_t z = __builtin_elementwise_add_sat(y, (u16x2_t){0x80, 0x80});
  return __builtin_bit_cast(unsigned, (u16x2_t)(z >> 15));
}
// bit of element e (0..3) of group g (0..3) in a lane's 16-bit word of a block: the low byte holds the even elements, the high byte
// the odd ones (the halves of the packed words, gathered without unpacking them)
__device__ __forceinline__ constexpr int keep_bit(int g, int e) { return 2 * g + (e >> 1) + 8 * (e & 1); }

// ---- the tile's outputs through LDS -----------------------------------------------------------------------------------------------
// The accumulator layout puts a ROW on each lane: stored from there, one 16-byte store instruction touches 32 rows x 32 B (32 cache
// lines, a quarter of each), and the CU's store path takes ~64 cycles for it: 17.5 B/clk/CU, 7,500 cycles for the 128 KiB of a tile
// (tools/store_path_bench.hip, shape 0); the same bytes as whole rows — 4 rows x 256 B per instruction — leave at 51 B/clk/CU (shape
// 1: 2,600 cycles).  The aux operand of the residual / mask epilogues came in the same row-per-lane shape with 8-byte loads, each behind
// its own predicate branch: ~10 us per tile (out-projection 34 us vs 24 us for the plain epilogue on the same problem).  So each wave
// owns an 8-KiB LDS region [32 rows][256 B] (16-byte chunk c of row r at r * 256 + ((c ^ (r & 15)) << 4): both access shapes are
// conflict-free or two-way) and, per 32-row block tm of its quadrant,
//   aux: eight 16-byte whole-row loads (issued two blocks ahead, range-checked buffer loads: no branches) -> region -> read back in the
//        accumulator layout;
//   out: finished and packed in the accumulator layout -> region (in place) -> read back as whole rows -> eight range-checked 16-byte
//        stores of 4 rows x 256 B.
// LDS operations of one wave execute in order, so the region needs no barrier and no wait between a write and the read behind it.
// CT: the epilogue's flag set (compile time; alpha = 1, no dropout).  The bias is not added here: it is what the tile's accumulators
// START from (bias_init below).  TN = 3: the wave tile is 96 columns, 12 of a row's 16 chunks; the lanes of chunks 12..15 get the
// out-of-range offset (their aux loads read zeros into region chunks nobody reads back, their stores are dropped).
// The keep-mask as bits (MMF_EPI_RELU_BITS / MMF_EPI_MASK_BITS, layout in mmfusion.h): a lane's sixteen values of a 32 x 32 block
// (tm, tn) are sixteen bits of ONE 16-bit word, and the block's 64 words lie together, so a wave writes or reads a block's bits
// with one 128-byte access straight from / into the accumulator layout: no aux tile, no LDS round trip.  The words are indexed by
// the PROBLEM's blocks (mb, nb are multiples of 32 at either tile width).  Range-checked like the rest: blocks past
// ceil(M / 32) rows fall behind the buffer, block columns past ceil(N / 32) get the out-of-range offset.
template <int CT, int TN>
__device__ __forceinline__ void drain_tile(const GemmArgs& args, const int pi, const mmf_gemm_problem& P, const int mb, const int nb,
                                           f32x16_t (&acc)[TN][4], char* region, const int lane) {
  constexpr bool AUX = (CT & (MMF_EPI_MASK_AUX | MMF_EPI_ADD_AUX)) != 0;
  constexpr bool DROP = (CT & MMF_EPI_DROPOUT) != 0;
  constexpr bool EMIT_BITS = (CT & MMF_EPI_RELU_BITS) != 0, MASK_BITS = (CT & MMF_EPI_MASK_BITS) != 0;
  static_assert(!(AUX && (EMIT_BITS || MASK_BITS)) && !(EMIT_BITS && MASK_BITS), "aux is one of: a bf16 tile, bits written, bits read");
  // dropout on the (activated) outputs, the mask of gemm6's epilogue: element m * N + n of the caller's problem `orig[pi]`
  const unsigned drop_key = DROP ? mmf_rng_key(*args.rng_state, args.site, (unsigned)args.orig[pi]) : 0u;
  const float drop_scale = DROP ? mmf_inv_keep(args.drop_thresh) : 1.f;
  const float alpha = (CT & (MMF_EPI_MASK_AUX | MMF_EPI_MASK_BITS)) ? args.alpha : 1.f;            // 1 / (1 - p) of a dropout backward rides on the ReLU mask
  const int r = lane & 31, h = lane >> 5, q = lane >> 4, cq = lane & 15;
  // region offsets: accumulator layout (8 bytes at chunk c = 4 tn + g, half h, of row r), whole-row layout (16-byte chunk cq of row 4 it + q)
  const unsigned wr_base = (unsigned)(r * 256 + 8 * h + 16 * (r & 15));
  const unsigned rd_base = (unsigned)(q * 256 + ((cq ^ q) << 4));
  auto acc_at = [&](int c) { return region + (wr_base ^ (unsigned)(c << 4)); };
  auto row_at = [&](int it) { return region + it * 1024 + (rd_base ^ (unsigned)((it & 3) << 6)); };
  // global side: lane's column chunk is fixed (8 bf16 at nb + 8 cq), its row walks 32 tm + 4 it + q.  Range-checked buffer accesses
  // against [base, last valid element]: rows past M fall outside; columns past N get an out-of-range offset.
  const bool col_ok = cq < 4 * TN && nb + 8 * cq < P.N;
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(P.C, 0, (int)((((long)P.M - 1) * P.ldc + P.N) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(AUX ? P.aux : P.C), 0,
                                                                       AUX ? (int)((((long)P.M - 1) * P.ldaux + P.N) * 2) : 0, 0x00020000);
  const unsigned c_off0 = col_ok ? (unsigned)(((long)(mb + q) * P.ldc + nb + 8 * cq) * 2) : 0x80000000u;
  const unsigned a_off0 = col_ok ? (unsigned)(((long)(mb + q) * P.ldaux + nb + 8 * cq) * 2) : 0x80000000u;
  const unsigned c_row4 = (unsigned)(4 * P.ldc * 2), a_row4 = (unsigned)(4 * P.ldaux * 2);

  // bits: 128 bytes per 32 x 32 block of the problem, row-major over its blocks; this lane's word of block (tm, tn) of the wave tile
  const int nb32 = (P.N + 31) >> 5;
  const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>((EMIT_BITS || MASK_BITS) ? P.aux : P.C), 0,
      (EMIT_BITS || MASK_BITS) ? ((P.M + 31) >> 5) * nb32 * 128 : 0, 0x00020000);
  auto bits_off = [&](int tm, int tn) {
    const int bn = (nb >> 5) + tn;
    return bn < nb32 ? (unsigned)((((mb >> 5) + tm) * nb32 + bn) * 128 + 2 * lane) : 0x80000000u;
  };
  unsigned keep[TN][4];                                       // MASK_BITS: the whole wave tile's words, loaded at the head of the drain
  if constexpr (MASK_BITS) {
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
        keep[tn][tm] = (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(brs, bits_off(tm, tn), 0, 0);
  }

  u32x4_t auxr[2][8];
  auto load_aux = [&](int tm, int slot) {
#pragma unroll
    for (int it = 0; it < 8; ++it)
      auxr[slot][it] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(ars, a_off0 + (unsigned)(8 * tm + it) * a_row4, 0, 0));
  };
  if constexpr (AUX) { load_aux(0, 0); load_aux(1, 1); }
  // (scheduling fences between the groups: without them the compiler hoists all 256 accumulator reads of the unrolled drain to its
  // head and spills what it cannot hold — accumulators included)
#pragma unroll
  for (int tm = 0; tm < 4; ++tm) {
    u32x2_t axv[TN][4];
    if constexpr (AUX) {
#pragma unroll
      for (int it = 0; it < 8; ++it) *reinterpret_cast<u32x4_t*>(row_at(it)) = auxr[tm & 1][it];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int g = 0; g < 4; ++g) axv[tn][g] = *reinterpret_cast<const u32x2_t*>(acc_at(4 * tn + g));
      __builtin_amdgcn_sched_barrier(0);
      if (tm + 2 < 4) load_aux(tm + 2, tm & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      // (the tile passes through an opaque statement HERE: its sixteen accumulator reads cannot be hoisted to the head of the drain,
      // where hipcc otherwise reads 160-250 accumulator registers into vector registers at once and spills the aux pieces in flight)
      asm volatile("" : "+a"(acc[tn][tm]));
      unsigned npos = 0;                                       // EMIT_BITS: NOT (stored bf16 value > 0); bit 2 g + i of each half: word i of group g
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4_t v = {acc[tn][tm][4 * g], acc[tn][tm][4 * g + 1], acc[tn][tm][4 * g + 2], acc[tn][tm][4 * g + 3]};
        // (the bit forms are not part of the shared statement: MMF_EPI_MASK_BITS applies its mask below, where MMF_EPI_MASK_AUX does inside)
        MMF_EPI_QUAD_CT(CT, v, axv[tn][g], (unsigned)(mb + 32 * tm + r) * (unsigned)P.N + (unsigned)(nb + 32 * tn + 8 * g + 4 * h),
                        drop_key, args.drop_thresh, drop_scale, alpha);
        if constexpr (MASK_BITS) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {                         // bit ? v * alpha : +0, the bit spread over the word as a mask
            // (as a statement the compiler cannot read: it turns every C form of this mask into and + compare + select, a
            // third more vector instructions per element than the aux form it replaces)
            int m;                                              // 0 / all ones
            asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(keep[tn][tm]), "s"(keep_bit(g, e)));
            v[e] = __uint_as_float(__float_as_uint(v[e] * alpha) & (unsigned)m);
          }
        }
        const u32x2_t w = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        if constexpr (EMIT_BITS) {                             // from the packed value: the predicate MASK_AUX applies to the stored tensor
          npos |= bf16x2_not_positive(w[0]) << (2 * g) | bf16x2_not_positive(w[1]) << (2 * g + 1);
        }
        *reinterpret_cast<u32x2_t*>(acc_at(4 * tn + g)) = w;
      }
      if constexpr (EMIT_BITS) __builtin_amdgcn_raw_buffer_store_b16((short)~((npos & 0xffu) | (npos >> 8)), brs, bits_off(tm, tn), 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    u32x4_t w[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) w[it] = *reinterpret_cast<const u32x4_t*>(row_at(it));
#pragma unroll
    for (int it = 0; it < 8; ++it) __builtin_amdgcn_raw_buffer_store_b128(w[it], crs, c_off0 + (unsigned)(8 * tm + it) * c_row4, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// CT: the launch's epilogue flag set, compile time (alpha = 1, no dropout, outputs in 8-column granularity: the host sends
// everything else to gemm6) — one drain form per kernel.
//
// ONE stage body serves every stage of every tile of the workgroup (the first form of this kernel instantiated the stage per role —
// tile's first, steady, descriptor switch, ring running dry, last — as gemm6 does; around the tile loop hipcc then copied the 256
// accumulator registers between the roles' code through vector registers and scratch).  What made the roles differ is removed:
//   * the accumulators never start from a zero C operand: sixteen MFMAs in front of the tile's first stage set them to the bias
//     (or to zero, from zero fragments);
//   * the ring never "runs dry": behind the workgroup's last tile the descriptors get a range of ZERO bytes, so the refills stay in
//     the instruction stream (and in the hand-overs' counts) but touch no memory — the range check answers them with zeros;
//   * the ring fill fetches NS - 1 stages and the late half of the NS-th, so the very first stage already finds its early pieces
//     to issue.
//
// CHAIN (K-segment chains, mmf_gemm_grouped_chain): an output tile's reduction runs over 1..4 segments whose operands live in different
// buffers.  A tile's segments are consecutive entries of the workgroup's walk, and a segment boundary is the tile hand-over above with
// two differences: the accumulators are kept (no bias_init) and nothing is drained.  The k-loop, the ring and the drain are the same
// code; every output element's MFMA chain is the bias start, then the k-substeps of segment 0, 1, .. in order.
template <bool B_KR, int CT, int TN, bool CHAIN>
__device__ __forceinline__ void gemm7_body(const GemmArgs& args, const int total_tiles, char* smem) {
  constexpr bool A_KR = false;
  using F = Form<TN>;
  constexpr int BNT = F::BNT, STAGE = F::STAGE, PPW = F::PPW, NMF = 4 * TN, NRD = 4 + TN;   // MFMAs / fragment reads per k-substep
  constexpr int WA = BK, WB = B_KR ? BNT : BK;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;                   // this wave's 128 x (32 TN) part of the tile
  const int nwg = gridDim.x;
  // The walk: round r hands ids r * nwg .. to the workgroups in ascending order when r is even and in DESCENDING order when it is odd.
  // The host sorts the problems by K, longest first, so ids run from the longest tiles to the shortest; the snake gives whoever got the
  // longest tiles of one round the shortest of the next (a static longest-processing-time deal).  With every round ascending, the in-projection
  // dgrad launch of the text group (192 tiles of 24 k-steps, 81 of 48: 273 tiles on 256 CUs) gave its 17 second-round tiles — long ones —
  // to workgroups 0 .. 16, four of which already held long tiles: 96 k-steps where 48 suffice (93 us in the step, 382 TF).
  const int wid = blockIdx.x;
  auto walk = [&](int round) { return round * nwg + ((round & 1) ? nwg - 1 - wid : wid); };
  TileSrc ns;
  TileDst cd, nd;
  int KT, lda, ldb;
  locate_tile<B_KR, TN, CHAIN>(args, total_tiles, walk(0), 0, ns, cd, lda, ldb);
  KT = ns.KT;

  // ---- LDS-DMA: this wave's PPW pieces of a stage (PPO of the m-operand, TN of the n-operand), per-lane source offsets for the tile
  // being FETCHED ----------------------------------------------------------------------------------------------------------------------
  unsigned voff[PPW], voffn[PPW];
  auto set_voff = [&](unsigned (&v)[PPW], int la, int lb) {
#pragma unroll
    for (int i = 0; i < PPO; ++i) v[i] = piece_voff<A_KR>(wave + 4 * i, la, lane);
#pragma unroll
    for (int i = 0; i < TN; ++i) v[PPO + i] = piece_voff<B_KR, BNT>(wave + 4 * i, lb, lane);
  };
  set_voff(voff, lda, ldb);
  char* const my_pieces = smem + wave * 1024;

  // The descriptors of the stage being fetched, as SCALARS (address low / high word, record bytes): carried across the tile loop as
  // <4 x i32> values they were given vector registers (their SGPR words copied into a VGPR quad at the loop header, which the "s"
  // operands of the LDS-DMA statements then printed: assembler errors); the quads are put together where they are used.
  struct Desc { int lo, hi, rec; };
  auto mkdesc = [](const unsigned short* p, int rec) {
    const unsigned long long a = (unsigned long long)(uintptr_t)p;
    return Desc{(int)(unsigned)a, (int)((unsigned)(a >> 32) & 0xffffu), rec};
  };
  auto advance = [](Desc& d, int bytes) {                    // one stage on; a range that is used up stays empty
    const unsigned long long a = (((unsigned long long)(unsigned)d.hi << 32) | (unsigned)d.lo) + (unsigned long long)bytes;
    d.lo = (int)(unsigned)a; d.hi = (int)(unsigned)(a >> 32);
    // (scalar asm: hipcc turns max(rec - bytes, 0) into a VECTOR saturating subtract, and a vector-computed descriptor word reaches the
    // "s" operand of the LDS-DMA statement as a VGPR — it inserts no readfirstlane there)
    int r;
    asm("s_sub_i32 %0, %1, %2\n\ts_max_i32 %0, %0, 0" : "=s"(r) : "s"(d.rec), "s"(bytes) : "scc");
    d.rec = r;
  };
  Desc dA = mkdesc(ns.Ab, ns.recA);
  Desc dB = mkdesc(ns.Bb, ns.recB);
  constexpr int stepA = BK * 2;
  int stepB = ns.stepB;                                      // bytes per stage of the tile being fetched
  const unsigned lds_pieces = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)my_pieces;
  auto hot_piece = [&](auto ic, const unsigned ring_base) {
    constexpr int I = decltype(ic)::value, OFF = I < PPO ? I * 4096 : TILE + (I - PPO) * 4096;
    const Desc& d = I < PPO ? dA : dB;
    const i32x4_t q = {d.lo, d.hi, d.rec, 0x00020000};
    // M0 (which the LDS-DMA reads) is the statement's output: a clobber of a reserved register is not honoured by the compiler.  One
    // wait state between the M0 write and the LDS-DMA that reads it, the s_nop (the hardware does not interlock them); it does not
    // depend on the number of pieces per stage.
    int m0w;
    asm volatile("s_add_i32 %0, %1, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds" : "={m0}"(m0w) : "s"(ring_base), "v"(voff[I]), "s"(q), "n"(OFF) : "memory");
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- the workgroup's one ring fill: NS - 1 stages and the late half of the NS-th (the same two-instruction pieces: no LDS-DMA the
  // compiler knows of, so the LDS accesses of drain_tile are never preceded by a compiler-placed vmcnt(0)) ---------------------------
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const unsigned rb = lds_pieces + (unsigned)(s * STAGE);
    hot_piece(std::integral_constant<int, 0>{}, rb); hot_piece(std::integral_constant<int, 1>{}, rb);
    hot_piece(std::integral_constant<int, 2>{}, rb); hot_piece(std::integral_constant<int, 3>{}, rb);
    if (s + 1 < NS) {
      hot_piece(std::integral_constant<int, 4>{}, rb); hot_piece(std::integral_constant<int, 5>{}, rb);
      hot_piece(std::integral_constant<int, 6>{}, rb);
      if constexpr (TN == 4) hot_piece(std::integral_constant<int, 7>{}, rb);
      advance(dA, stepA); advance(dB, stepB);                // afterwards: stage NS - 1, the one being fetched
    }
  }

  // The entry behind the one in (ns, nd) — the same tile's next segment (CHAIN), else the first segment of the workgroup's next
  // tile — becomes what the fetch side switches to; false: the walk has ended, the refills get an empty range.
  int nround = 0, nseg = 0;
  nd = cd;
#pragma unroll
  for (int i = 0; i < PPW; ++i) voffn[i] = voff[i];
  auto locate_next = [&]() {
    if (CHAIN && !nd.last) {
      ++nseg;
    } else {
      ++nround;
      nseg = 0;
      if (walk(nround) >= total_tiles) {
        ns.recA = 0; ns.recB = 0; ns.stepB = 0;
        return false;
      }
    }
    int la, lb;
    locate_tile<B_KR, TN, CHAIN>(args, total_tiles, walk(nround), nseg, ns, nd, la, lb);
    set_voff(voffn, la, lb);
    return true;
  };
  bool has_next = locate_next();

  // ---- fragment addressing (tile-independent) ----------------------------------------------------------------------------------------
  unsigned la0, la1, lb0, lb1;
  Frag4<A_KR>::lane_parts(WA, lane, la0, la1);
  Frag4<B_KR>::lane_parts(WB, lane, lb0, lb1);
  const unsigned smem_base = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)smem;
  const unsigned qa = (unsigned)((WA / 32) * 2048 * 4 * wm);
  const unsigned qb = (unsigned)(B_KR ? 512 * TN * wn : (WB / 32) * 2048 * TN * wn);   // column blocks / row blocks TN wn ..
  la0 += smem_base + qa; la1 += smem_base + qa;
  lb0 += smem_base + TILE + qb; lb1 += smem_base + TILE + qb;

  f32x16_t acc[TN][4];                // [tn][tm]; set to the bias (or to zero) by bias_init in front of every tile

  // Bias.  In the accumulator layout a lane would hold 64 bias values per tile (columns nb + 32 tn + 8 g + 4 h + e) through the
  // drain, on top of the aux pieces in flight: with them the drain spills.  Instead the tile's accumulators START from the bias: lane
  // r keeps ONE value per 32-column block tn (bias[nb + 32 tn + r], loaded a tile ahead: at the head of the previous tile's drain) and
  // 4 TN MFMAs spread them as outer products with a ones fragment,
  //     D[n][m] = sum_k A[n][k] B[k][m],  A[n][0..2] = the exact three-way bf16 split of bias[n],  B[0..2][m] = 1
  // (exact in f32: 8 + 8 + 8 mantissa bits; attention2.hip does the same with its row statistics).  16 of a K = 768 tile's 784 MFMAs.
  constexpr bool use_bias = (CT & MMF_EPI_BIAS) != 0;
  float bcur[TN] = {};
  auto load_bias = [&](float (&b)[TN], const TileDst& d) {
    const mmf_gemm_problem& P = args.p[d.pi];
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.bias), 0, P.N * 4, 0x00020000);
    const unsigned off = (unsigned)((d.n0 + 32 * TN * wn + (lane & 31)) * 4);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)                              // (the builtin returns the 32 bits as an integer)   past N: 0
      b[tn] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b32(brs, off + (unsigned)(32 * tn * 4), 0, 0));
  };
  auto split3 = [&](float x) {
    const bool lo = lane < 32;
    const unsigned hh = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(hh);
    const unsigned mm = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(mm);
    const unsigned ll = __float_as_uint(r2) & 0xffff0000u;
    const u32x4_t w = {lo ? ((hh >> 16) | mm) : 0u, lo ? (ll >> 16) : 0u, 0u, 0u};
    return __builtin_bit_cast(bf16x8_t, w);
  };
  auto bias_init = [&](const float (&b)[TN]) {
    const f32x16_t zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const u32x4_t ow = {lane < 32 ? 0x3f803f80u : 0u, lane < 32 ? 0x00003f80u : 0u, 0u, 0u};
    // one opaque copy of the ones fragment per row block: 4 TN MFMAs with the same operands would be merged into four (or, without
    // a bias, into ONE) and their results copied into the other accumulator tiles register by register
    u32x4_t ones[4] = {ow, ow, ow, ow};
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) asm volatile("" : "+v"(ones[tm]));
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      u32x4_t bw = __builtin_bit_cast(u32x4_t, use_bias ? split3(b[tn]) : __builtin_bit_cast(bf16x8_t, u32x4_t{0u, 0u, 0u, 0u}));
      asm volatile("" : "+v"(bw));
#pragma unroll
      for (int tm = 0; tm < 4; ++tm) {
        acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, bw), __builtin_bit_cast(bf16x8_t, ones[tm]), zero, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  if constexpr (use_bias) load_bias(bcur, cd);

  // The vmcnt counts (hand-counted: the pieces are inline asm, the compiler counts none of them).  Per wave a stage is PPW = 4 + TN
  // pieces: PPO = 4 "late" ones of the m-operand and TN "early" ones of the n-operand (8 at TN = 4, 7 at TN = 3).  In issue order:
  //   ring fill:        stages 0 .. NS - 2 whole (PPW each), then the late PPO of stage NS - 1;
  //   stage g, step 0:  the early TN of stage g + NS - 1;     stage g, step 1 behind the hand-over: the late PPO of stage g + NS.
  // First wait, stage 0 complete: younger than its last piece are stages 1 .. NS - 2 and the late part of NS - 1,
  //   PPW * (NS - 2) + PPO  (20 at TN = 4, 18 at TN = 3).
  // Hand-over in stage g (needs stage g + 1): the last piece of stage g + 1 is its early part, issued in step 0 of stage g - NS + 2 (in
  // the ring fill while that is negative).  Younger, up to the hand-over in step 1 of stage g: the late parts of stages g + 2 ..
  // g + NS - 1 and their early parts, NS - 2 of each,
  //   (NS - 2) * (PPO + TN) = PPW * (NS - 2)  (16 at TN = 4, 14 at TN = 3).
  // Anything else the wave issues (bias, aux loads and stores of a drain) is younger than the pieces it is counted with: the wait
  // then covers more than it needs, never less.
  vm_wait<PPW * (NS - 2) + PPO>();    // stage 0 landed (with the bias loads behind the pieces this waits for more: once per workgroup)
  __builtin_amdgcn_s_barrier();
  Frag4<A_KR> fa[2];
  Frag4<B_KR, TN> fb[2];
  fa[0].template issue<WA, 0, 0>(la0, la1);
  fb[0].template issue<WB, 0, 0>(lb0, lb1);
  frag_wait(fa[0], fb[0]);

  auto mf = [&](const Frag4<A_KR>& a, const Frag4<B_KR, TN>& b, int i) {
    const int tm = i / TN, tn = i % TN;
    acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b.get(tn), a.get(tm), acc[tn][tm], 0, 0, 0);
    // an empty statement that "uses" the tile: the MFMA builtin has no side effect, and in this kernel instruction selection sank the
    // sixteen MFMAs of a substep below the reads and pieces that are written between them (each down to its next use, the same
    // tile's MFMA of the following substep); the volatile statement chains it into the order of the other asm statements
    asm volatile("" ::"a"(acc[tn][tm]));
    __builtin_amdgcn_sched_barrier(0);
  };

  // One stage (gemm6.hip's schedule, BK = 32: two k-substeps of NMF = 4 TN MFMAs and NRD = 4 + TN fragment reads).  g: the workgroup's running stage count (ring slot
  // g % NS).  kt == ksw: this is stage KT - NS of its tile — from its hand-over on the refills fetch the NEXT tile (or nothing).
  // The hand-over counts PIECES only.  Stores, aux and bias loads of a drain may be younger than the pieces waited for: the wait
  // then covers more than it needs (safe whether or not the hardware retires loads and stores in one order), never less.
  auto stage = [&](const unsigned g, const int kt, const int ksw) {
    unsigned long long swmask;
    const Desc nA = mkdesc(ns.Ab, ns.recA), nB = mkdesc(ns.Bb, ns.recB);
    const unsigned so = (g % NS) * STAGE;
    const unsigned ring_cur = lds_pieces + so, ring_prev = lds_pieces + ((g + NS - 1) % NS) * STAGE;
    // substep 0: MFMA i (i < NRD) is followed by one read of substep 1's fragments; the early pieces (the n-operand part of the stage
    // whose m-operand part went out at the end of the previous stage) ride behind MFMAs NRD, NRD + 2, .. (8, 10, 12, 14 | 7, 9, 11)
#pragma unroll
    for (int i = 0; i < NMF; ++i) {
      mf(fa[0], fb[0], i);
      if (i < NRD) MMF_G6_READ(TN, fa[1], fb[1], 1, i, so);
      if (i == NRD)     hot_piece(std::integral_constant<int, 4>{}, ring_prev);
      if (i == NRD + 2) hot_piece(std::integral_constant<int, 5>{}, ring_prev);
      if (i == NRD + 4) hot_piece(std::integral_constant<int, 6>{}, ring_prev);
      if constexpr (TN == 4) { if (i == NRD + 6) hot_piece(std::integral_constant<int, 7>{}, ring_prev); }
    }
    frag_wait(fa[1], fb[1]);
    // substep 1: four MFMAs, the stage hand-over, then MFMAs 4 .. NRD + 3 each followed by one read of the next stage's first fragments
    // and the last four MFMAs by the late pieces (12..15 | 8..11: at TN = 3 the last three carry a read and a piece)
    const unsigned sn = ((g + 1) % NS) * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) mf(fa[1], fb[1], i);
    vm_wait<PPW * (NS - 2)>();
    __builtin_amdgcn_s_barrier();                              // the next stage landed for everyone; nobody reads this one any more
    __builtin_amdgcn_sched_barrier(0);
    // Behind the hand-over: advance the descriptors, or switch them (and the per-lane offsets) to the next tile's first stage — as
    // SELECTS, not as a branch (with a branch here hipcc duplicated the rest of the stage into both arms and joined the two copies'
    // 256 accumulator registers with v_accvgpr_mov chains behind the k-loop), in four portions of at most nine instructions behind
    // MFMAs 4..7 (a wave issues eight instructions per 32-cycle MFMA).  The selects are inline asm: ONE compare feeds all of them
    // (hipcc re-derived the condition per portion: 45 instructions), and left to itself it computes all of it between the vmcnt
    // wait and the barrier, in front of an idle matrix pipe.
#pragma unroll
    for (int i = 4; i < NMF; ++i) {
      mf(fa[1], fb[1], i);
      if (i < 4 + NRD) MMF_G6_READ(TN, fa[0], fb[0], 0, i - 4, sn);
      if (i == 4) {                                            // both descriptors one stage on (eight scalar instructions)
        advance(dA, stepA);
        advance(dB, stepB);
        asm volatile("" ::"s"(dA.lo), "s"(dA.hi), "s"(dA.rec), "s"(dB.lo), "s"(dB.hi), "s"(dB.rec));
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i == 5) {                                            // one compare, seven scalar selects, the lane mask for the vector selects
        asm volatile("s_cmp_eq_u32 %8, %16\n\t"
                     "s_cselect_b32 %0, %9, %0\n\ts_cselect_b32 %1, %10, %1\n\ts_cselect_b32 %2, %11, %2\n\t"
                     "s_cselect_b32 %3, %12, %3\n\ts_cselect_b32 %4, %13, %4\n\ts_cselect_b32 %5, %14, %5\n\t"
                     "s_cselect_b32 %6, %15, %6\n\ts_cselect_b64 %7, -1, 0"
                     : "+s"(dA.lo), "+s"(dA.hi), "+s"(dA.rec), "+s"(dB.lo), "+s"(dB.hi), "+s"(dB.rec), "+s"(stepB), "=s"(swmask)
                     : "s"(kt), "s"(nA.lo), "s"(nA.hi), "s"(nA.rec), "s"(nB.lo), "s"(nB.hi), "s"(nB.rec), "s"(ns.stepB), "s"(ksw)
                     : "scc");
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i == 6) {
        asm volatile("v_cndmask_b32_e64 %0, %0, %4, %8\n\tv_cndmask_b32_e64 %1, %1, %5, %8\n\t"
                     "v_cndmask_b32_e64 %2, %2, %6, %8\n\tv_cndmask_b32_e64 %3, %3, %7, %8"
                     : "+v"(voff[0]), "+v"(voff[1]), "+v"(voff[2]), "+v"(voff[3])
                     : "v"(voffn[0]), "v"(voffn[1]), "v"(voffn[2]), "v"(voffn[3]), "s"(swmask));
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i == 7) {
        if constexpr (TN == 4)
          asm volatile("v_cndmask_b32_e64 %0, %0, %4, %8\n\tv_cndmask_b32_e64 %1, %1, %5, %8\n\t"
                       "v_cndmask_b32_e64 %2, %2, %6, %8\n\tv_cndmask_b32_e64 %3, %3, %7, %8"
                       : "+v"(voff[4]), "+v"(voff[5]), "+v"(voff[6]), "+v"(voff[7])
                       : "v"(voffn[4]), "v"(voffn[5]), "v"(voffn[6]), "v"(voffn[7]), "s"(swmask));
        else
          asm volatile("v_cndmask_b32_e64 %0, %0, %3, %6\n\tv_cndmask_b32_e64 %1, %1, %4, %6\n\t"
                       "v_cndmask_b32_e64 %2, %2, %5, %6"
                       : "+v"(voff[4]), "+v"(voff[5]), "+v"(voff[6])
                       : "v"(voffn[4]), "v"(voffn[5]), "v"(voffn[6]), "s"(swmask));
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i == NMF - 4) hot_piece(std::integral_constant<int, 0>{}, ring_cur);
      if (i == NMF - 3) hot_piece(std::integral_constant<int, 1>{}, ring_cur);
      if (i == NMF - 2) hot_piece(std::integral_constant<int, 2>{}, ring_cur);
      if (i == NMF - 1) hot_piece(std::integral_constant<int, 3>{}, ring_cur);
    }
    frag_wait(fa[0], fb[0]);
  };

  char* const region = smem + NS * STAGE + wave * 8192;
  unsigned g = 0;
  for (;;) {
    bias_init(bcur);
    for (;;) {
      const int ksw = KT - NS;                                 // >= 1 (host)
      for (int kt = 0; kt < KT; ++kt, ++g) stage(g, kt, ksw);
      if (!CHAIN || cd.last) break;
      cd = nd;                                                 // the tile's next segment: the hand-over of stage ksw switched the fetch side to it
      KT = ns.KT;
      has_next = locate_next();
    }
    // ---- the tile's outputs ----------------------------------------------------------------------------------------------------------
    const mmf_gemm_problem& P = args.p[cd.pi];
    const int mb = cd.m0 + 128 * wm, nb = cd.n0 + 32 * TN * wn;
    if constexpr (use_bias) { if (has_next) load_bias(bcur, nd); }   // the NEXT tile's bias: the drain covers the round trip
#ifndef MMF_G7_NODRAIN
    drain_tile<CT & ~MMF_EPI_BIAS, TN>(args, cd.pi, P, mb, nb, acc, region, lane);
#else
    if (lane == 0 && mb == -1) static_cast<volatile unsigned short*>(P.C)[0] = (unsigned short)acc[0][0][0];   // (ablation: the tile is not stored)
#endif
    if (!has_next) break;
    cd = nd;
    KT = ns.KT;
    has_next = locate_next();
  }
  vm_wait<0>();                       // the zero-range refills behind the last tile
}

template <bool B_KR, int CT, int TN, bool CHAIN>
__global__ __launch_bounds__(NTHREADS, 1)
void gemm7_persistent_kernel(const GemmArgs args, const int total_tiles) {
  // the ring and, behind it, one 8-KiB output staging region per wave: all 160 KiB of the CU at TN = 4, 144 KiB at TN = 3
  __shared__ __attribute__((aligned(1024))) char smem[Form<TN>::LDS];
  gemm7_body<B_KR, CT, TN, CHAIN>(args, total_tiles, smem);
}

// The instantiated forms, one line each: the (layout, flag set) pairs of the fusion step's NT / NN launches and of the chain form (NN:
// the input gradient summed over the linears that read one input).  A line answers "is there such a form" and, given a table (a), launches it.
template <bool B_KR, int CT, bool CHAIN>
void launch7(const GemmArgs& a, int total, int grid, int tile_n, hipStream_t s) {
  if (tile_n == 192) hipLaunchKernelGGL((gemm7_persistent_kernel<B_KR, CT, 3, CHAIN>), dim3(grid), dim3(NTHREADS), 0, s, a, total);
  else               hipLaunchKernelGGL((gemm7_persistent_kernel<B_KR, CT, 4, CHAIN>), dim3(grid), dim3(NTHREADS), 0, s, a, total);
}
#define MMF_G7_FORM(LAYOUT, CHAIN, FLAGS)                                                        \
  if (layout == (LAYOUT) && chain == (CHAIN) && eflags == (FLAGS)) {                             \
    if (a) launch7<(LAYOUT) == MMF_GEMM_NN, (FLAGS), CHAIN>(*a, total, grid, tile_n, s);         \
    return true;                                                                                 \
  }
constexpr int RB = MMF_EPI_RELU | MMF_EPI_RELU_BITS;           // the ReLU forms that also write the keep-mask as bits
bool launch7_select(int layout, int eflags, bool chain, const GemmArgs* a = nullptr, int total = 0, int grid = 0, hipStream_t s = nullptr, int tile_n = 256) {
  MMF_G7_FORM(MMF_GEMM_NT, false, 0)                                                        // plain NT
  MMF_G7_FORM(MMF_GEMM_NT, false, MMF_EPI_BIAS)                                             // in-projections
  MMF_G7_FORM(MMF_GEMM_NT, false, MMF_EPI_BIAS | MMF_EPI_RELU)                              // FFN1
  MMF_G7_FORM(MMF_GEMM_NT, false, MMF_EPI_BIAS | MMF_EPI_ADD_AUX)                           // out-projection and FFN2 (residual)
  MMF_G7_FORM(MMF_GEMM_NT, false, MMF_EPI_BIAS | MMF_EPI_RELU | MMF_EPI_DROPOUT)            // FFN hidden layer in training mode
  MMF_G7_FORM(MMF_GEMM_NT, false, RB)                                                       // FFN hidden layer of a forward that will be
  MMF_G7_FORM(MMF_GEMM_NT, false, RB | MMF_EPI_BIAS)                                        // differentiated
  MMF_G7_FORM(MMF_GEMM_NT, false, RB | MMF_EPI_DROPOUT)
  MMF_G7_FORM(MMF_GEMM_NT, false, RB | MMF_EPI_BIAS | MMF_EPI_DROPOUT)
  MMF_G7_FORM(MMF_GEMM_NN, false, 0)                                                        // dgrads
  MMF_G7_FORM(MMF_GEMM_NN, false, MMF_EPI_BIAS)                                             // (the chain form's twin)
  MMF_G7_FORM(MMF_GEMM_NN, false, MMF_EPI_MASK_AUX)                                         // dH (ReLU mask)
  MMF_G7_FORM(MMF_GEMM_NN, false, MMF_EPI_MASK_BITS)
  MMF_G7_FORM(MMF_GEMM_NN, false, MMF_EPI_ADD_AUX)                                          // dX (residual gradient)
  MMF_G7_FORM(MMF_GEMM_NN, true, 0)
  MMF_G7_FORM(MMF_GEMM_NN, true, MMF_EPI_BIAS)
  MMF_G7_FORM(MMF_GEMM_NN, true, MMF_EPI_ADD_AUX)
  return false;
}
#undef MMF_G7_FORM
}  // namespace

static int g_persistent_wgs = [] { const char* e = getenv("MMF_GEMM7_WGS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 0; }();
extern "C" int mmf_gemm_set_persistent_workgroups(int n) {
  if (n < 0 || n > 65536) MMF_FAIL(MMF_E_SHAPE, "mmf_gemm_set_persistent_workgroups: %d not in 0..65536", n);
  g_persistent_wgs = n;
  return MMF_OK;
}
static int g_tile_n = 0;                                       // 0: automatic (pick_tile_n), else 256 / 192 for every launch
static thread_local int t_last_tile_n = 0;
extern "C" int mmf_gemm7_set_tile_n(int n) {
  if (n != 0 && n != 256 && n != 192) MMF_FAIL(MMF_E_SHAPE, "mmf_gemm7_set_tile_n: %d is not 0, 256 or 192", n);
  g_tile_n = n;
  return MMF_OK;
}
extern "C" int mmf_gemm7_last_tile_n(void) { return t_last_tile_n; }

namespace {
int persistent_grid_cap() {
  static const int cus = [] { int c = mmf_device_cu_count(); return c > 0 ? c : 256; }();
  return g_persistent_wgs > 0 ? g_persistent_wgs : cus;
}
// order: the problems longest K first (the kernel's problem order)
int tiles_of(const mmf_gemm_problem& p, int bn) { return ((p.M + BM - 1) / BM) * ((p.N + bn - 1) / bn); }
// The launch's makespan on min(tiles, cap) workgroups at tile width bn, in units of K x bn per tile: the kernel's walk (snake rounds
// over the XCD-aware tile order, gemm7_body / mmf_xcd_tile) replayed on the host, the longest workgroup's sum.
long long walk_makespan(const mmf_gemm_problem* problems, const int* order, int n, int bn, int cap, int granule) {
  int start[MMF_GEMM_MAX_PROBLEMS + 1];
  start[0] = 0;
  for (int i = 0; i < n; ++i) start[i + 1] = start[i] + tiles_of(problems[order[i]], bn);
  const int total = start[n], grid = total < cap ? total : cap;
  if (total == 0) return 0;
  static thread_local std::vector<long long> load;
  load.assign(grid, 0);
  for (int o = 0; o < total; ++o) {
    const int round = o / grid, pos = o % grid, wid = (round & 1) ? grid - 1 - pos : pos;
    const int bid = mmf_xcd_tile(o, total, granule);
    const int pi = (int)(std::upper_bound(start, start + n + 1, bid) - start) - 1;
    load[wid] += (long long)problems[order[pi]].K * bn;
  }
  return *std::max_element(load.begin(), load.end());
}
// Tile width of a launch: 192 only where its makespan is strictly shorter than at 256 (a tie keeps 256: fewer, larger tiles).
// Replaying the walk costs 15-55 us of host time for the step's launches (one pass per tile and width), which an eager step would
// pay per launch; the answers are remembered per thread for the last 16 launch shapes (the step has ten).
struct TileNMemo {
  int cap, granule, n, width;
  int mnk[3 * MMF_GEMM_MAX_PROBLEMS];
};
int pick_tile_n(const mmf_gemm_problem* problems, const int* order, int n, int cap) {
  const int granule = mmf_xcd_granule();
  static thread_local TileNMemo memo[16];
  static thread_local int used = 0, next = 0;
  TileNMemo key;
  key.cap = cap; key.granule = granule; key.n = n;
  for (int i = 0; i < n; ++i) {
    const mmf_gemm_problem& p = problems[order[i]];
    key.mnk[3 * i] = p.M; key.mnk[3 * i + 1] = p.N; key.mnk[3 * i + 2] = p.K;
  }
  for (int e = 0; e < used; ++e) {
    const TileNMemo& m = memo[e];
    if (m.cap == cap && m.granule == granule && m.n == n && std::equal(key.mnk, key.mnk + 3 * n, m.mnk)) return m.width;
  }
  key.width = walk_makespan(problems, order, n, 192, cap, granule) < walk_makespan(problems, order, n, 256, cap, granule) ? 192 : 256;
  memo[next] = key;
  next = (next + 1) % 16;
  if (used < 16) ++used;
  return key.width;
}
void sort_by_k(const mmf_gemm_problem* problems, int n, int* order) {      // longest reduction first (see the walk in gemm7_body)
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order, order + n, [&](int x, int y) { return problems[x].K > problems[y].K; });
}
}  // namespace

extern "C" int mmf_gemm7_tile_n(const mmf_gemm_problem* problems, int num_problems, int workgroups) {
  if (!problems || num_problems < 1 || num_problems > MMF_GEMM_MAX_PROBLEMS || workgroups < 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_gemm7_tile_n: %d problems, %d workgroups", num_problems, workgroups);
  int order[MMF_GEMM_MAX_PROBLEMS];
  sort_by_k(problems, num_problems, order);
  return pick_tile_n(problems, order, num_problems, workgroups > 0 ? workgroups : persistent_grid_cap());
}

// What generation 7 takes of ONE problem (mmf_gemm7_supports asks it per problem, the chain form per segment): the ring's K, outputs and
// aux rows in 8-column granularity, a 16-byte aligned aux; with the bit forms aux is the bit buffer (no ldaux) and has to be there.
static bool gemm7_takes(const mmf_gemm_problem& p, int epilogue) {
  const bool bits = (epilogue & (MMF_EPI_RELU_BITS | MMF_EPI_MASK_BITS)) != 0;
  if (p.K % BK || p.K < (NS + 1) * BK || (p.N & 7) || (p.ldc & 7)) return false;
  if (p.aux && ((!bits && (p.ldaux & 7)) || !mmf_aligned16(p.aux))) return false;
  return !bits || p.aux;
}
// whether the persistent kernel can take this launch (gemm.hip asks before selecting it)
bool mmf_gemm7_supports(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue, int out_f32, const mmf_gemm_extra* extra) {
  if (out_f32 || !launch7_select(layout, epilogue, false)) return false;
  if (extra && extra->alpha != 1.f && !(layout == MMF_GEMM_NN && (epilogue == MMF_EPI_MASK_AUX || epilogue == MMF_EPI_MASK_BITS))) return false;   // alpha rides on the mask only
  if ((epilogue & MMF_EPI_DROPOUT) && !(extra && extra->rng_state)) return false;
  for (int i = 0; i < num_problems; ++i)
    if (!gemm7_takes(problems[i], epilogue)) return false;
  return true;
}

int mmf_gemm7_launch(const mmf_gemm_problem* problems, int num_problems, int layout, int epilogue,
                     int out_f32, const mmf_gemm_extra* extra, hipStream_t s) {
  if (!mmf_gemm7_supports(problems, num_problems, layout, epilogue, out_f32, extra))
    MMF_FAIL(MMF_E_UNSUPPORTED, "mmf_gemm_grouped: the persistent kernel takes NT / NN launches with bf16 output, K %% 32 == 0, K >= %d, N and the "
             "leading dimensions of C / aux multiples of 8, and the flag sets of the fusion step (alpha only with the NN ReLU mask)", (NS + 1) * BK);
  int order[MMF_GEMM_MAX_PROBLEMS];
  sort_by_k(problems, num_problems, order);
  const int cap = persistent_grid_cap();
  const int tile_n = g_tile_n ? g_tile_n : pick_tile_n(problems, order, num_problems, cap);
  GemmArgs a;
  mmf_gemm_table_begin(a, epilogue, extra);
  for (int i = 0; i < num_problems; ++i) {
    const mmf_gemm_problem& p = problems[order[i]];
    if (const int e = mmf_gemm_table_add(a, p, tiles_of(p, tile_n), order[i], layout, true)) return e;
    a.orig[i] = (short)order[i];
  }
  const int total = a.tile_start[num_problems], grid = total < cap ? total : cap;
  t_last_tile_n = tile_n;
  launch7_select(layout, epilogue, false, &a, total, grid, s, tile_n);
  MMF_CHECK_LAUNCH("mmf_gemm_grouped(v7)");
  return MMF_OK;
}

// ---- K-segment chains (mmf_gemm_grouped_chain) ------------------------------------------------------------------------------------------
int mmf_gemm_problem_fault(const mmf_gemm_problem& p, int layout, int epilogue, char* why, size_t why_bytes);   // gemm.hip: the entry points' rules

namespace {
static_assert(MMF_GEMM_MAX_CHAINS * MMF_GEMM_CHAIN_MAX_SEGMENTS <= MMF_GEMM_MAX_PROBLEMS, "a launch's segments fill GemmArgs::p at most");
// the chains as the walk and pick_tile_n see them: one problem of K = the sum of the segments' K each
void chains_as_problems(const mmf_gemm_chain* chains, int n, mmf_gemm_problem* out) {
  for (int i = 0; i < n; ++i) {
    out[i] = mmf_gemm_problem{};
    out[i].M = chains[i].M;
    out[i].N = chains[i].N;
    for (int j = 0; j < chains[i].num_segments; ++j) out[i].K += chains[i].seg[j].K;
  }
}
// a chain's segments as the problems the kernel walks -> their number.  bias and aux only under their flags: what the launch does not read is not looked at
int chain_segments(const mmf_gemm_chain& c, int epilogue, mmf_gemm_problem* out) {
  for (int j = 0; j < c.num_segments; ++j) {
    const mmf_gemm_segment& g = c.seg[j];
    out[j] = mmf_gemm_problem{g.A, g.B, c.C, (epilogue & MMF_EPI_BIAS) ? c.bias : nullptr, (epilogue & MMF_EPI_ADD_AUX) ? c.aux : nullptr,
                              c.M, c.N, g.K, g.lda, g.ldb, c.ldc, c.ldaux};
  }
  return c.num_segments;
}
// What is about chains: their number, a chain's number of segments, a residual of the output's shape.  Every segment is a problem
// the entry points' rules hold for, that generation 7 takes, and whose A, B, C and aux fit the drain's and the ring's descriptors.
bool chain_shapes_ok(const mmf_gemm_chain* chains, int n, int epilogue) {
  if (!chains || n < 1 || n > MMF_GEMM_MAX_CHAINS) return false;
  for (int i = 0; i < n; ++i) {
    const mmf_gemm_chain& c = chains[i];
    if (c.num_segments < 1 || c.num_segments > MMF_GEMM_CHAIN_MAX_SEGMENTS) return false;
    if ((epilogue & MMF_EPI_ADD_AUX) && c.ldaux < c.N) return false;
    mmf_gemm_problem seg[MMF_GEMM_CHAIN_MAX_SEGMENTS];
    chain_segments(c, epilogue, seg);
    for (int j = 0; j < c.num_segments; ++j)
      if (mmf_gemm_problem_fault(seg[j], MMF_GEMM_NN, epilogue, nullptr, 0) != MMF_OK || !gemm7_takes(seg[j], epilogue) ||
          !mmf_gemm_descriptors_fit(seg[j], MMF_GEMM_NN, epilogue, true))
        return false;
  }
  return true;
}
}  // namespace

extern "C" int mmf_gemm7_chain_tile_n(const mmf_gemm_chain* chains, int num_chains, int workgroups) {
  if (!chain_shapes_ok(chains, num_chains, 0) || workgroups < 0)
    MMF_FAIL(MMF_E_SHAPE, "mmf_gemm7_chain_tile_n: %d chains, %d workgroups, or a chain the chain form does not take", num_chains, workgroups);
  mmf_gemm_problem sums[MMF_GEMM_MAX_CHAINS];
  chains_as_problems(chains, num_chains, sums);
  return mmf_gemm7_tile_n(sums, num_chains, workgroups);
}

// whether the persistent kernel's chain form takes this launch: an instantiated form, every segment a problem generation 7 takes
bool mmf_gemm7_chain_supports(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue) {
  return launch7_select(layout, epilogue, true) && chain_shapes_ok(chains, num_chains, epilogue);
}

int mmf_gemm7_chain_launch(const mmf_gemm_chain* chains, int num_chains, int layout, int epilogue, hipStream_t s) {
  if (!mmf_gemm7_chain_supports(chains, num_chains, layout, epilogue))
    MMF_FAIL(MMF_E_SHAPE, "mmf_gemm_grouped_chain: takes 1..%d NN chains of 1..%d segments with bf16 output, the flag sets none / MMF_EPI_BIAS / "
             "MMF_EPI_ADD_AUX, every segment's K %% 32 == 0 and >= %d, N and the leading dimensions multiples of 8, 16-byte aligned operands "
             "(mmf_gemm_chain_available)", MMF_GEMM_MAX_CHAINS, MMF_GEMM_CHAIN_MAX_SEGMENTS, (NS + 1) * BK);
  mmf_gemm_problem sums[MMF_GEMM_MAX_CHAINS];
  chains_as_problems(chains, num_chains, sums);
  int order[MMF_GEMM_MAX_CHAINS];
  sort_by_k(sums, num_chains, order);                          // longest total reduction first
  const int cap = persistent_grid_cap();
  const int tile_n = g_tile_n ? g_tile_n : pick_tile_n(sums, order, num_chains, cap);
  // a unit of the table is a chain: orig[i] is where chain i's segments start in p[] (gemm6_parts.h)
  GemmArgs a;
  mmf_gemm_table_begin(a, epilogue, nullptr);
  int nseg = 0;
  for (int i = 0; i < num_chains; ++i) {
    a.orig[mmf_gemm_table_unit(a, tiles_of(sums[order[i]], tile_n))] = (short)nseg;
    nseg += chain_segments(chains[order[i]], epilogue, a.p + nseg);
  }
  a.orig[num_chains] = (short)nseg;
  const int total = a.tile_start[num_chains], grid = total < cap ? total : cap;
  t_last_tile_n = tile_n;
  launch7_select(layout, epilogue, true, &a, total, grid, s, tile_n);
  MMF_CHECK_LAUNCH("mmf_gemm_grouped_chain(v7)");
  return MMF_OK;
}
