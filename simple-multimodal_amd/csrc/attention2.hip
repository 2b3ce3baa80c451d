// Grouped fused attention (forward, dQ, dK/dV): fat workgroups, LDS-DMA ring, one dual-use LDS image.
//
// Structure (measurements behind each choice in DESIGN.md section 5 and profiles/r03_attn_*):
//   * all attention problems of a stage (the six cross blocks, or the three self-attentions, of a MulT pass — unequal
//     Tq / Tk) go out as ONE launch; workgroup ids are remapped so that the chunks of one (b, h) (and neighbouring heads
//     of one batch row) run on the SAME XCD (blockIdx % 8) and share its L2;
//   * products are oriented so that every probability tile stays in registers between its two uses: forward / dQ compute
//     S^T = K.Q^T (query on the lane: row max / sum / LSE / delta are per-lane scalars, P^T feeds O^T = V^T.P^T and dS^T
//     feeds dQ^T = K^T.dS^T from the accumulator), dK/dV computes S = Q.K^T (key on the lane; a wave keeps dK^T, dV^T
//     of its 32 keys in accumulators while the workgroup sweeps the queries; no atomics, deterministic);
//   * swept tiles (K/V in forward and dQ; Q/dO/LSE/delta in dK/dV) go HBM/L2 -> LDS by LDS-DMA into a 2-stage ring, the
//     next tile in flight under the current tile's MFMAs; rows past T come back as zeros from the buffer range check;
//   * softmax on raw scores, p = exp2(fma(s, c, -m)); the running maximum is raised only when a row's block maximum
//     exceeds it by 2^DEFER (guide T13), 32-key blocks, blocks that hold only padding are skipped;
//   * transposed operands by asm ds_read_b64_tr_b16 with counted lgkmcnt waits;
//   * ONE LDS image for row reads and transposed reads (attn_helpers.h: 8-row x 32-column subtiles, XOR swizzle) instead
//     of 16-byte padded rows: the transposed reads were 2-way bank-conflicted, and the LDS port is as busy as the matrix
//     pipe in these kernels (~1 KiB of fragment reads per MFMA);
//   * prologue loads (Q; Q, dO, O; K, V) issued together behind one wait instead of 6 / 18 / 12 serial round trips;
//   * per-lane LDS-DMA source offsets computed once per wave, tiles addressed through per-tile descriptors (SALU only).
#include "attn2_common.h"

namespace {

// MMF_ATTN_STAMPS (build-time, measurement only; tools/attn2_bwd_stamps.py): s_memtime cycles per wave and segment of the
// backward kernels.  0 prologue, 1 vmcnt wait, 2 barrier, 3 DMA issue, 4 S / dP products, 5 P / dS arithmetic,
// 6 dQ^T (dQ kernel) or dV^T / dK^T (dK/dV kernel) chain, 7 epilogue, 8 HW_ID.  Every stamp drains the wave's LDS reads
// (s_memtime returns through lgkmcnt), so the segments are attributions, not the undisturbed schedule.
#ifdef MMF_ATTN_STAMPS
__device__ unsigned long long* g_bstamps = nullptr;       // [kernel 0 dQ / 1 dKdV][workgroup][4 waves][12]
#define BSTAMP(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); seg[i] += t_ - tlast; tlast = t_; } while (0)
#define BSTAMP_DECL unsigned long long seg[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long tlast = __builtin_readcyclecounter()
#define BSTAMP_STORE(kern) do { seg[8] = __builtin_amdgcn_s_getreg(63492); \
    if (g_bstamps && (threadIdx.x & 63) == 0) { for (int i_ = 0; i_ < 12; ++i_) \
      g_bstamps[(((size_t)(kern) * 65536 + blockIdx.x) * 4 + (threadIdx.x >> 6)) * 12 + i_] = seg[i_]; } } while (0)
#else
#define BSTAMP(i) do {} while (0)
#define BSTAMP_DECL do {} while (0)
#define BSTAMP_STORE(kern) do {} while (0)
#endif

// One wave of the forward: its 32-row query block at rows qs (ACTIVE), or staging and barriers only.
template <int DH, bool DROP, bool ACTIVE>
__device__ __forceinline__ void fwd2_wave(const AttnArgs2& a, const mmf_attn_problem& P, const int pidx, const int bh,
                                          const int qs, char* smem) {
  constexpr int KS = DH / 16, DT = DH / 32, TILE_B = img_tile_bytes<DH>(), STAGE_B = 2 * TILE_B;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tq = P.Tq, Tk = P.Tk, H = P.H;
  const int b = bh / H, h = bh % H;

  // (the (b, h) origin b * T * ld + h * DH is spelled out at each use on purpose: formed by a function, with any parameter passing,
  // the leading dimension is loaded ahead of the product and 20 of the 22 kernels come out in another instruction order)
  const unsigned short* Kg = static_cast<const unsigned short*>(P.K) + (size_t)b * Tk * P.ldk + h * DH;
  const unsigned short* Vg = static_cast<const unsigned short*>(P.V) + (size_t)b * Tk * P.ldv + h * DH;
  TileDma<DH> dma;
  dma.init(P.ldk, P.ldv, wave, lane);
  auto issue = [&](int j) {
    dma.issue(Kg + (size_t)64 * j * P.ldk, Vg + (size_t)64 * j * P.ldv, P.ldk, P.ldv, Tk - 64 * j, smem + (j & 1) * STAGE_B, wave);
  };
  const int ntiles = (Tk + 63) / 64;
  issue(0);

  // Q fragments through the wave's slice of stage 1 (free until the loop issues tile 1 behind its first barrier)
  char* slice = smem + STAGE_B + wave * img_slice_bytes<DH>();
  bf16x8_t qf[KS];
  if constexpr (ACTIVE) {
    const unsigned short* Qg = static_cast<const unsigned short*>(P.Q) + (size_t)b * Tq * P.ldq + h * DH;
    RowLoad<DH> rl;
    rl.issue(rows_rsrc(Qg, 0, Tq, P.ldq), P.ldq, qs, lane);
    rl.commit(qf, lane, slice);
  }

  f32x16_t o[DT];
  float m = NEG_BIG, l = 0.f;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = zero16();
  const float c = a.scale * LOG2E;
  const unsigned dkey = DROP ? mmf_rng_key(*a.rng_state, a.site, (unsigned)(pidx * 4096 + bh) + a.stream_base) : 0u;
  // (these three are repeated in every body on purpose: held in a struct that hands out tr_base, 20 kernels change)
  const unsigned tlo = tr_lane_lo(lane), thi = tr_lane_hi(lane);
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  for (int j = 0; j < ntiles; ++j) {
    ring_handover(j, ntiles, issue, [](int) {});
    if constexpr (ACTIVE) {
      const char* sK = smem + (j & 1) * STAGE_B;
      const TrBase vaV = tr_base(smem_lds + (j & 1) * STAGE_B + TILE_B, tlo, thi);
      const int kb = j * 64;
      // one 32-key block: S^T = K.Q^T (raw scores), online softmax (lane = query), O^T += V^T.P^T
      auto block = [&](auto KTc) {
        constexpr int KT = decltype(KTc)::value;
        const int k0 = kb + 32 * KT;
        if (k0 >= Tk) return;                              // wave-uniform: nothing but masked keys
        f32x16_t s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        // all KS fragment reads in flight before the first MFMA: one exposed LDS latency per block instead of KS / 2
        bf16x8_t kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = row_frag<DH>(sK, 32 * KT, ks, lane);
        __builtin_amdgcn_sched_barrier(0);                 // (the scheduler otherwise re-pairs them with the MFMAs)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);                 // the asm V^T reads below are invisible to the compiler's lgkmcnt count
        constexpr int TD = FWD_TRDEPTH;
        s16x4_t lo[2 * DT], hi[2 * DT];
        PvStepD<DH, KT, TD, 0>::prime(vaV, lo, hi);
        if (k0 + 32 > Tk) {                                // ragged block
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            s[r] = key < Tk ? s[r] : NEG_BIG;
          }
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = half_max(mx) * c;
        if (!__all(mx <= m + DEFER)) {                     // wave-uniform: raise the running maximum
          const float mnew = fmaxf(m, mx);
          const float alpha = fast_exp2(m - mnew);
          m = mnew;
          l *= alpha;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
        const float nm = -m;
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fast_exp2(__builtin_fmaf(s[r], c, nm));
          s[r] = p;
          rs += p;
        }
        l += rs;
        if (DROP) {          // nn.MultiheadAttention(dropout=p): drop/rescale the probabilities fed to P.V only
          const unsigned qidx = (unsigned)(qs + (lane & 31)) * (unsigned)Tk;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const unsigned key = (unsigned)(k0 + (r & 3) + 8 * (r >> 2) + 4 * half);
            s[r] = mmf_keep(dkey, qidx + key, a.drop_thresh) ? s[r] * a.inv_keep : 0.f;
          }
        }
        bf16x8_t pf;
        PvStepD<DH, KT, TD, 0>::run(vaV, lo, hi, s, pf, o);
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
    }
  }

  if constexpr (ACTIVE) {
    // the stage the last tile did not use is free (every wave passed the last barrier): reuse the wave's slice there
    char* oslice = smem + (ntiles & 1) * STAGE_B + wave * img_slice_bytes<DH>();
    unsigned short* Og = static_cast<unsigned short*>(P.O) + (size_t)b * Tq * P.ldo + h * DH;
    const float lt = half_sum(l);
    const int lane_e = lane_again();
    store_rows_lds<DH>(o, 1.f / lt, Og, P.ldo, qs, Tq, lane_e, oslice);
    const int qrow = qs + (lane & 31);
    if (half == 0 && qrow < Tq) P.LSE[(size_t)bh * Tq + qrow] = m * LN2 + __logf(lt);
  }
}

// One 32-row query block per wave (128 rows per workgroup), <= 168 registers, so THREE workgroups share a CU (3 x 48 KiB
// of LDS) and a wave's LDS / MFMA dependency waits have two other waves on its SIMD to hide under (round 2: against two
// blocks per wave at two workgroups per CU, 102.3 -> 91.7 us per step).
template <int DH, bool DROP>
__global__ __launch_bounds__(NT, 3)
void attn_fwd2n_kernel(const AttnArgs2 a) {
  constexpr int STAGE_B = 2 * img_tile_bytes<DH>();
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];
  MMF_ATTN_WG_DECODE(a, a.rpc[pi], q0);                     // rpc <= 128 here
  const int nb = (min(P.Tq, q0 + rpc) - q0 + 31) >> 5;      // 32-row query blocks in this chunk (1..4)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qs = q0 + 32 * wave, pidx = a.orig[pi];
  // (the two instantiations are named in every kernel on purpose: chosen through a generic lambda, the head_dim 96 kernels change)
  if (wave < nb) fwd2_wave<DH, DROP, true>(a, P, pidx, bh, qs, smem);
  else           fwd2_wave<DH, DROP, false>(a, P, pidx, bh, qs, smem);
}

// ================================================================================================
// Backward: the dQ kernel (which also writes delta), then the dK/dV kernel; P is recomputed from LSE; no atomics,
// deterministic.  The swept tiles — K/V in the dQ kernel, Q/dO (+ LSE, delta) in the dK/dV kernel — ride the same 2-stage
// LDS-DMA ring as the forward's: fetched through registers, and in the dK/dV kernel only AFTER the MFMAs, every tile
// cost one exposed HBM/L2 latency, which made the x30 problems (one active wave walking 8 tiles) 37-41 us each.
// ================================================================================================

// dQ^T += K^T . dS^T for block KT: PvStep with the K tile as the transposed operand.
// ACTIVE false: the wave only stages tiles and joins the barriers.  (The sweep split of the dK/dV kernel below was tried here
// too — waves 0 and 1 sharing the 32 query rows of a x30 problem — and taken out again: at this kernel's 168-register budget
// (three waves per SIMD) a third instantiation of the body spilled 31 registers instead of 6, a runtime selector 66, and the
// spills land in the main path's loop.)
// GIVEN: delta is an input (mmf_attn_bwd_grouped_delta: the caller computed it in f32, mmf_attn_delta_f32); O is not read.
// GIVEN with DROP (mmf_attn_bwd_grouped_delta_keyed): that delta is the dropped one, sum_j p_ij w_ij dp_ij.
template <int DH, bool DROP, bool ACTIVE, bool GIVEN = false>
__device__ __forceinline__ void dq2_wave(const AttnArgs2& a, const mmf_attn_problem& P, const int pidx, const int bh,
                                         const int qs, char* smem) {
  constexpr int KS = DH / 16, DT = DH / 32, TILE_B = img_tile_bytes<DH>(), STAGE_B = 2 * TILE_B;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tq = P.Tq, Tk = P.Tk, H = P.H;
  const int b = bh / H, h = bh % H;
  const unsigned short* Kg = static_cast<const unsigned short*>(P.K) + (size_t)b * Tk * P.ldk + h * DH;
  const unsigned short* Vg = static_cast<const unsigned short*>(P.V) + (size_t)b * Tk * P.ldv + h * DH;
  TileDma<DH> dma;
  dma.init(P.ldk, P.ldv, wave, lane);
  auto issue = [&](int j) {
    dma.issue(Kg + (size_t)64 * j * P.ldk, Vg + (size_t)64 * j * P.ldv, P.ldk, P.ldv, Tk - 64 * j, smem + (j & 1) * STAGE_B, wave);
  };
  const int ntiles = (Tk + 63) / 64;
  BSTAMP_DECL;
  issue(0);

  const int qrow = qs + (lane & 31);
  const size_t qoff = (size_t)b * Tq * P.ldq + h * DH, ooff = (size_t)b * Tq * P.ldo + h * DH;
  char* slice = smem + STAGE_B + wave * img_slice_bytes<DH>();
  bf16x8_t qf[KS], dof[KS];
  float delta = 0.f, lse2 = 0.f;
  if constexpr (ACTIVE) {
    auto rsrc = [&](const void* base, size_t off, int ld) { return rows_rsrc(base, off, Tq, ld); };
    if constexpr (GIVEN) {
      RowLoad<DH> rq, rdo;
      rq.issue(rsrc(P.Q, qoff, P.ldq), P.ldq, qs, lane);
      rdo.issue(rsrc(P.dO, ooff, P.ldo), P.ldo, qs, lane);
      rq.commit(qf, lane, slice);
      rdo.commit(dof, lane, slice);
      delta = qrow < Tq ? P.delta[(size_t)bh * Tq + qrow] : 0.f;
    } else {
    RowLoad<DH> rq, rdo, ro;                                  // 3 x 6 loads in flight, one wait (RowLoad, attn_helpers.h)
    rq.issue(rsrc(P.Q, qoff, P.ldq), P.ldq, qs, lane);
    rdo.issue(rsrc(P.dO, ooff, P.ldo), P.ldo, qs, lane);
    ro.issue(rsrc(P.O, ooff, P.ldo), P.ldo, qs, lane);
    rq.commit(qf, lane, slice);
    rdo.commit(dof, lane, slice);
    bf16x8_t of[KS];
    ro.commit(of, lane, slice);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) delta = dot8(delta, __builtin_bit_cast(u32x4_t, of[ks]), __builtin_bit_cast(u32x4_t, dof[ks]));
    delta = half_sum(delta);
    if (half == 0 && qrow < Tq) P.delta[(size_t)bh * Tq + qrow] = delta;
    }
    lse2 = (qrow < Tq ? P.LSE[(size_t)bh * Tq + qrow] : 0.f) * LOG2E;
  }
  const float c = a.scale * LOG2E;
  const unsigned dkey = DROP ? mmf_rng_key(*a.rng_state, a.site, (unsigned)(pidx * 4096 + bh) + a.stream_base) : 0u;
  const unsigned qidx = (unsigned)qrow * (unsigned)Tk;
  f32x16_t dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = zero16();
  const unsigned tlo = tr_lane_lo(lane), thi = tr_lane_hi(lane);
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  if constexpr (ACTIVE) BSTAMP(0);
  for (int j = 0; j < ntiles; ++j) {
    ring_handover(j, ntiles, issue, [&](int i) { if constexpr (ACTIVE) BSTAMP(i); });
    if constexpr (ACTIVE) BSTAMP(3);
    if constexpr (ACTIVE) {
      const char* sK = smem + (j & 1) * STAGE_B;
      const char* sV = sK + TILE_B;
      const TrBase vaK = tr_base(smem_lds + (j & 1) * STAGE_B, tlo, thi);
      auto block = [&](auto KTc) {
        constexpr int KT = decltype(KTc)::value;
        const int k0 = j * 64 + 32 * KT;
        if (k0 >= Tk) return;
        f32x16_t s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<DH>(sK, 32 * KT, ks, lane), qf[ks], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<DH>(sV, 32 * KT, ks, lane), dof[ks], dp, 0, 0, 0);
        }
        BSTAMP(4);
        constexpr int TD = DQ_TRDEPTH;
        s16x4_t lo[2 * DT], hi[2 * DT];
        PvStepD<DH, KT, TD, 0>::prime(vaK, lo, hi);         // the first K^T fragments land under the dS arithmetic
        const bool ragged = k0 + 32 > Tk;
        f32x16_t ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = fast_exp2(__builtin_fmaf(s[r], c, -lse2));
          const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (ragged) p = key < Tk ? p : 0.f;
          float dpv = dp[r];                                // d(P_dropped) -> dP through the same mask
          if (DROP) dpv = mmf_keep(dkey, qidx + (unsigned)key, a.drop_thresh) ? dpv * a.inv_keep : 0.f;
          ds[r] = p * (dpv - delta);                        // dS^T (scale applied at the store)
        }
        BSTAMP(5);
        bf16x8_t pf;
        PvStepD<DH, KT, TD, 0>::run(vaK, lo, hi, ds, pf, dq);
        BSTAMP(6);
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
    }
  }
  if constexpr (ACTIVE) {
    char* oslice = smem + (ntiles & 1) * STAGE_B + wave * img_slice_bytes<DH>();
    const int lane_e = lane_again();
    store_rows_lds<DH>(dq, a.scale, static_cast<unsigned short*>(P.dQ) + qoff, P.ldq, qs, Tq, lane_e, oslice);
    BSTAMP(7);
    BSTAMP_STORE(0);
  }
}

template <int DH, bool DROP, bool GIVEN = false>
__global__ __launch_bounds__(NT, DQ_WAVES_PER_SIMD)
void attn_bwd_dq2_kernel(const AttnArgs2 a) {
  constexpr int STAGE_B = 2 * img_tile_bytes<DH>();
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];
  MMF_ATTN_WG_DECODE(a, ROWS_PER_WG, q0);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qs = q0 + 32 * wave, pidx = a.orig[pi];
  if (qs < P.Tq) dq2_wave<DH, DROP, true, GIVEN>(a, P, pidx, bh, qs, smem);
  else           dq2_wave<DH, DROP, false, GIVEN>(a, P, pidx, bh, qs, smem);
}

// Row statistics of the dK/dV kernel through the matrix pipe (round 3).  In S = Q.K^T the key is the lane and the query row
// the accumulator register, so LSE and delta of a 32-row block are needed as 16 different values per lane.  Rounds 1-2
// staged them in LDS and read them back with eight broadcast ds_read_b128 per block in the middle of the P / dS
// arithmetic: four or five exposed LDS round trips per block (the "arith" segment of the stamped dK/dV kernel was 3x the
// dQ kernel's, profiles/r03_attn_bwd_stamps.txt) and a quarter of the kernel's LDS cycles.  Instead each lane keeps the two
// statistics of ITS OWN row (lane & 31) of the block in a register (prefetched from global memory one tile ahead) and
// ONE MFMA per statistic spreads them into the accumulator layout as an outer product with a ones fragment:
//     D[q][key] = sum_k A[q][k] B[k][key],  A[q][0..2] = the exact three-way bf16 split of x[q],  B[0..2][key] = 1,
// exact in f32 (8 + 8 + 8 mantissa bits, f32 accumulate).  With D as the initial accumulator of the S (and, without
// dropout, the dP) chain the subtraction is free:  S' = Q.K^T - LSE / scale,  p = exp2(c S');  dP' = dO.V^T - delta,
// dS = p dP'.
// Sweep split (split_wg; sel = the wave's half, -1 without the split): a problem with <= 32 keys gives them to waves 0 and 1,
// wave w works on 32-row query block w of every tile; wave 1's partial dK^T, dV^T are added to wave 0's through LDS at the end.
template <int DH, bool DROP, bool ACTIVE>
__device__ __forceinline__ void dkv2_wave(const AttnArgs2& a, const mmf_attn_problem& P, const int pidx, const int bh,
                                          const int k0, char* smem, const bool split_wg, const int sel) {
  constexpr int KS = DH / 16, DT = DH / 32, TILE_B = img_tile_bytes<DH>(), STAGE_B = 2 * TILE_B;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tq = P.Tq, Tk = P.Tk, H = P.H;
  const int b = bh / H, h = bh % H;
  const unsigned short* Qg = static_cast<const unsigned short*>(P.Q) + (size_t)b * Tq * P.ldq + h * DH;
  const unsigned short* dOg = static_cast<const unsigned short*>(P.dO) + (size_t)b * Tq * P.ldo + h * DH;
  const __amdgpu_buffer_rsrc_t rsL = f32_rsrc(P.LSE + (size_t)bh * Tq, Tq), rsD = f32_rsrc(P.delta + (size_t)bh * Tq, Tq);
  TileDma<DH> dma;
  dma.init(P.ldq, P.ldo, wave, lane);
  auto issue = [&](int j) {
    dma.issue(Qg + (size_t)64 * j * P.ldq, dOg + (size_t)64 * j * P.ldo, P.ldq, P.ldo, Tq - 64 * j, smem + (j & 1) * STAGE_B, wave);
  };
  float st_l[2], st_d[2];                                    // LSE, delta of this lane's row of the two blocks of tile j (row_stats)
  auto stats = [&](int j) { row_stats<false>(rsL, rsD, j, lane, Tq, st_l, st_d); };
  const int ntiles = (Tq + 63) / 64;
  BSTAMP_DECL;
  issue(0);
  if constexpr (ACTIVE) stats(0);

  const size_t koff = (size_t)b * Tk * P.ldk + h * DH, voff = (size_t)b * Tk * P.ldv + h * DH;
  char* slice = smem + STAGE_B + wave * img_slice_bytes<DH>();
  bf16x8_t kf[KS], vf[KS];
  if constexpr (ACTIVE) {
    const __amdgpu_buffer_rsrc_t rsK = rows_rsrc(P.K, koff, Tk, P.ldk), rsV = rows_rsrc(P.V, voff, Tk, P.ldv);
    RowLoad<DH> rk, rv;                                       // 2 x 6 loads in flight, one wait (RowLoad, attn_helpers.h)
    rk.issue(rsK, P.ldk, k0, lane);
    rv.issue(rsV, P.ldv, k0, lane);
    rk.commit(kf, lane, slice);
    rv.commit(vf, lane, slice);
  }
  f32x16_t dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) { dk[dt] = zero16(); dv[dt] = zero16(); }
  const float c = a.scale * LOG2E;
  const unsigned dkey = DROP ? mmf_rng_key(*a.rng_state, a.site, (unsigned)(pidx * 4096 + bh) + a.stream_base) : 0u;
  const unsigned kcol = (unsigned)(k0 + (lane & 31));
  const unsigned tlo = tr_lane_lo(lane), thi = tr_lane_hi(lane);
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  if constexpr (ACTIVE) BSTAMP(0);
  for (int j = 0; j < ntiles; ++j) {
    ring_handover(j, ntiles, issue, [&](int i) { if constexpr (ACTIVE) BSTAMP(i); });
    if constexpr (ACTIVE) BSTAMP(3);
    if constexpr (ACTIVE) {
      const char* sQ = smem + (j & 1) * STAGE_B;
      const char* sdO = sQ + TILE_B;
      // this tile's row statistics as MFMA operands; the next tile's are requested now and land under this tile's work
      const float nls = -1.f / a.scale;
      const float cl[2] = {st_l[0] * nls, st_l[1] * nls}, cd[2] = {-st_d[0], -st_d[1]};
      const bf16x8_t one3 = ones3_frag(half == 0);
      if (j + 1 < ntiles) stats(j + 1);
      const TrBase vaQ = tr_base(smem_lds + (j & 1) * STAGE_B, tlo, thi), vadO = tr_base(smem_lds + (j & 1) * STAGE_B + TILE_B, tlo, thi);
      auto block = [&](auto QSc) {
        constexpr int QS = decltype(QSc)::value;
        const int q0 = j * 64 + 32 * QS;
        if (q0 >= Tq) return;
        if (sel >= 0 && QS != sel) return;                 // sweep split: this wave's half of the tile
        f32x16_t s, dp, z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        s = spread_rows(cl[QS], half == 0, one3, z);   // S' starts at -LSE / scale
        f32x16_t dm;                                                                      // -delta[q] in every key column
        dm = spread_rows(cd[QS], half == 0, one3, z);
        if constexpr (DROP) dp = z; else dp = dm;                                         // dP' starts at -delta (no dropout)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<DH>(sQ, 32 * QS, ks, lane), kf[ks], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<DH>(sdO, 32 * QS, ks, lane), vf[ks], dp, 0, 0, 0);
        }
        BSTAMP(4);
        constexpr int TD = DKV_TRDEPTH;
        s16x4_t lo[4 * DT], hi[4 * DT];
        DkvStepD<DH, QS, TD, 0>::prime(vaQ, vadO, lo, hi);  // the first fragments land under the P / dS arithmetic
        f32x16_t ds;
        unsigned qbase = (unsigned)(q0 + 4 * half) * (unsigned)Tk + kcol;
        if constexpr (DROP) asm volatile("" : "+v"(qbase));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fast_exp2(s[r] * c);
          if constexpr (DROP) {
            // element index q * Tk + key as one per-block lane value + a scalar multiple of Tk: written as (q0 + c_r + 4 half) * Tk + key,
            // hipcc hoists the sixteen (c_r + 4 half) * Tk + key out of the sweep and spills them (40 registers, reloaded every block)
            const bool keep = mmf_keep(dkey, qbase + (unsigned)((r & 3) + 8 * (r >> 2)) * (unsigned)Tk, a.drop_thresh);
            s[r] = keep ? p * a.inv_keep : 0.f;                                       // dV^T += dO^T . P_dropped
            ds[r] = p * ((keep ? dp[r] * a.inv_keep : 0.f) + dm[r]);
          } else {
            s[r] = p;
            ds[r] = p * dp[r];
          }
        }
        BSTAMP(5);
        bf16x8_t pf, dsf;
        DkvStepD<DH, QS, TD, 0>::run(vaQ, vadO, lo, hi, s, ds, pf, dsf, dv, dk);
        BSTAMP(6);
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
    }
  }
  if (split_wg) {                                        // wave 1's partial sums -> wave 0 (the free stage holds them)
    float* red = reinterpret_cast<float*>(smem + (ntiles & 1) * STAGE_B);
    if (ACTIVE && sel == 1) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          red[(dt * 16 + r) * 64 + lane] = dk[dt][r];
          red[((DT + dt) * 16 + r) * 64 + lane] = dv[dt][r];
        }
    }
    __syncthreads();
    if (ACTIVE && sel == 0) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          dk[dt][r] += red[(dt * 16 + r) * 64 + lane];
          dv[dt][r] += red[((DT + dt) * 16 + r) * 64 + lane];
        }
    }
    __syncthreads();
  }
  if constexpr (ACTIVE) {
    if (sel > 0) return;
    char* oslice = smem + (ntiles & 1) * STAGE_B + wave * img_slice_bytes<DH>();
    const int lane_e = lane_again();
    store_rows_lds<DH>(dk, a.scale, static_cast<unsigned short*>(P.dK) + koff, P.ldk, k0, Tk, lane_e, oslice);
    store_rows_lds<DH>(dv, 1.f, static_cast<unsigned short*>(P.dV) + voff, P.ldv, k0, Tk, lane_e, oslice);
    BSTAMP(7);
    BSTAMP_STORE(1);
  }
}

template <int DH, bool DROP>
__global__ __launch_bounds__(NT, 2)      // dK^T, dV^T, K and V fragments alone are 144 registers: two waves per SIMD
void attn_bwd_dkv2_kernel(const AttnArgs2 a) {
  constexpr int STAGE_B = 2 * img_tile_bytes<DH>();
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];
  MMF_ATTN_WG_DECODE(a, ROWS_PER_WG, kc0);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = kc0 + 32 * wave, pidx = a.orig[pi];
  const bool split = P.Tk <= 32;                            // workgroup-uniform: the sweep split (dkv2_wave)
  const bool act = split ? wave < 2 : k0 < P.Tk;
  if (act) dkv2_wave<DH, DROP, true>(a, P, pidx, bh, split ? kc0 : k0, smem, split, split ? wave : -1);
  else     dkv2_wave<DH, DROP, false>(a, P, pidx, bh, k0, smem, split, -1);
}

// ================================================================================================
// Uniform backward (mmf_attn_bwd_grouped_uniform): every query row of a batch row has the SAME output gradient u[b] — the
// attention output is consumed only through its mean over T.  With u_h the head's columns of u[b]:
//     c[k]     = V[k,:] . u_h           dP[q][k] = c[k] for every q: one dot product per KEY instead of a Tq x Tk product
//     delta[q] = O[q,:] . u_h
//     dS[q][k] = P[q][k] (c[k] - delta[q])
//     dQ = scale dS K      dK = scale dS^T Q      dV[k,:] = (sum_q P[q][k]) u_h           (rank one)
// Three launches: a streaming kernel for c (V read once), then the dQ kernel, which forms delta from its own O rows as dq2_wave
// does (a first form took delta from the streaming kernel too: 22.6 us for that launch; one stream runs the launches in turn anyway),
// then the dK/dV kernel.  Against dq2_wave / dkv2_wave: no dP chain in either, no dV chain, the ring carries ONE tile per stage
// (K; Q), and the prologue loads Q and O; K.  The bodies are separate functions: the general ones are at their register budgets.
// LDS: the two one-tile stages first, then the four wave-private slices of the prologue / epilogue (nothing of the ring is reused).
// ================================================================================================
struct UniArgs {
  AttnArgs2 a;
  const float* c[MMF_ATTN_MAX_PROBLEMS];      // c of a.p[i], f32 [B*H*Tk]
};

// dK^T += Q^T . dS for the 32 query rows of block QS of the Q tile: the one chain DkvStepD keeps here is PvStepD's sequence
// (fragment n = k-substep n / DT, d-tile n % DT) with the Q tile as the transposed operand.
template <int DH, int QS, int D, int N> using DkStepD = PvStepD<DH, QS, D, N>;
constexpr int UNI_TRDEPTH = 2;

// c of problem i: c[(b*H + h)*Tk + k] = V[b*Tk + k][h*DH ..] . u[b][h*DH ..] in f32.  A workgroup takes STAT_CHUNKS consecutive 16-byte
// chunks of the matrix' (row, chunk) grid, one chunk per lane and pass (fully coalesced), leaves each chunk's partial sum in LDS and
// adds the DH/8 partial sums of a (row, head): STAT_CHUNKS is a multiple of DH/8 as a row's chunk count is, so no head straddles.
constexpr int STAT_THREADS = 256, STAT_PASSES = 6, STAT_CHUNKS = STAT_THREADS * STAT_PASSES;
struct StatArgs {
  int nprob;
  int blk_start[MMF_ATTN_MAX_PROBLEMS + 1];
  // g != nullptr (mmf_attn_bwd_grouped_pooled): u is not given but made here, u[b][:] = bf16(g[b][:] * inv) (meanpool_bwd_body's
  // rounding), used, and written by the lanes that hold row t = 0 of a batch row
  struct Job { const unsigned short* x; const unsigned short* u; float* out; int B, H, T, ldx, ldu; const unsigned short* g; int ldg; float inv; } j[MMF_ATTN_MAX_PROBLEMS];
};
template <int DH>
__global__ __launch_bounds__(STAT_THREADS)
void attn_uniform_stats_kernel(const StatArgs a) {
  constexpr int CPH = DH / 8, NG = STAT_CHUNKS / CPH;
  static_assert(STAT_CHUNKS % CPH == 0, "a head's chunks must not straddle two workgroups");
  __shared__ float part[STAT_CHUNKS];
  const int ji = mmf_group_problem(a.blk_start, a.nprob, blockIdx.x);
  const StatArgs::Job& J = a.j[ji];
  const unsigned blk = (unsigned)((int)blockIdx.x - a.blk_start[ji]);
  const unsigned cpr = (unsigned)(J.H * CPH), nchunks = (unsigned)(J.B * J.T) * cpr;      // (the host checked the range)
  u32x4_t x[STAT_PASSES], u[STAT_PASSES];
#pragma unroll
  for (int i = 0; i < STAT_PASSES; ++i) {
    const unsigned idx = blk * STAT_CHUNKS + threadIdx.x + STAT_THREADS * i;
    x[i] = u[i] = u32x4_t{0u, 0u, 0u, 0u};
    if (idx < nchunks) {
      const unsigned row = idx / cpr, ch = idx - row * cpr, b = row / (unsigned)J.T;
      x[i] = *reinterpret_cast<const u32x4_t*>(J.x + (size_t)row * J.ldx + ch * 8);
      if (J.g) {
        const u32x4_t w = *reinterpret_cast<const u32x4_t*>(J.g + (size_t)b * J.ldg + ch * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) u[i][e] = pack_bf16x2(bf16lo(w[e]) * J.inv, bf16hi(w[e]) * J.inv);
        if (row == b * (unsigned)J.T) *reinterpret_cast<u32x4_t*>(const_cast<unsigned short*>(J.u) + (size_t)b * J.ldu + ch * 8) = u[i];
      } else {
        u[i] = *reinterpret_cast<const u32x4_t*>(J.u + (size_t)b * J.ldu + ch * 8);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < STAT_PASSES; ++i) {
    float s = 0.f;                                            // (dot8's text on purpose: through the function this kernel changes)
#pragma unroll
    for (int e = 0; e < 4; ++e) s += bf16lo(x[i][e]) * bf16lo(u[i][e]) + bf16hi(x[i][e]) * bf16hi(u[i][e]);
    part[threadIdx.x + STAT_THREADS * i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NG) {
    const unsigned g = blk * NG + threadIdx.x;                // (row, head) pair
    if (g < (unsigned)(J.B * J.T * J.H)) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < CPH; ++e) s += part[threadIdx.x * CPH + e];
      const unsigned row = g / (unsigned)J.H, h = g - row * J.H, b = row / (unsigned)J.T, t = row - b * J.T;
      J.out[((size_t)b * J.H + h) * J.T + t] = s;
    }
  }
}

// One wave of the uniform dQ kernel: dq2_wave<.., GIVEN> without the dP chain, the V tile and the dO rows.  dP^T[key][q] = c[key]
// reaches the accumulator layout (key on the register, query on the lane) the way the dK/dV kernel spreads its row statistics: one
// outer-product MFMA of the exact three-way split of this lane's c[k0 + (lane & 31)] with a ones fragment; the two values of a tile
// are requested one tile ahead (they land behind the next hand-over's wait).
template <int DH, bool ACTIVE>
__device__ __forceinline__ void dq2u_wave(const AttnArgs2& a, const mmf_attn_problem& P, const float* cst, const int bh,
                                          const int qs, char* smem) {
  constexpr int KS = DH / 16, DT = DH / 32, TILE_B = img_tile_bytes<DH>();
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tq = P.Tq, Tk = P.Tk, H = P.H;
  const int b = bh / H, h = bh % H;
  const unsigned short* Kg = static_cast<const unsigned short*>(P.K) + (size_t)b * Tk * P.ldk + h * DH;
  const __amdgpu_buffer_rsrc_t rsC = f32_rsrc(cst + (size_t)bh * Tk, Tk);
  TileDma<DH> dma;
  dma.init(P.ldk, P.ldk, wave, lane);
  auto issue = [&](int j) { dma.issue_x(Kg + (size_t)64 * j * P.ldk, P.ldk, Tk - 64 * j, smem + (j & 1) * TILE_B, wave); };
  float ck[2];                                               // c of this lane's key of the two blocks of tile j (keys past Tk read as 0)
  auto cstat = [&](int j) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
      ck[kt] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsC, (unsigned)(64 * j + 32 * kt + (lane & 31)) * 4u, 0, 0));
  };
  const int ntiles = (Tk + 63) / 64;
  issue(0);
  if constexpr (ACTIVE) cstat(0);

  const int qrow = qs + (lane & 31);
  const size_t qoff = (size_t)b * Tq * P.ldq + h * DH;
  char* slice = smem + 2 * TILE_B + wave * img_slice_bytes<DH>();
  bf16x8_t qf[KS];
  float delta = 0.f, lse2 = 0.f;
  if constexpr (ACTIVE) {
    const __amdgpu_buffer_rsrc_t rsQ = rows_rsrc(P.Q, qoff, Tq, P.ldq);
    const size_t ooff = (size_t)b * Tq * P.ldo + h * DH;
    const __amdgpu_buffer_rsrc_t rsO = rows_rsrc(P.O, ooff, Tq, P.ldo);
    RowLoad<DH> rq, ro;                                       // 2 x 6 loads in flight, one wait (RowLoad, attn_helpers.h)
    rq.issue(rsQ, P.ldq, qs, lane);
    ro.issue(rsO, P.ldo, qs, lane);
    rq.commit(qf, lane, slice);
    bf16x8_t of[KS];
    ro.commit(of, lane, slice);
    // delta = O . u_h as dq2_wave forms O . dO, against the one row; written for the dK/dV kernel behind this one
    const unsigned short* ug = static_cast<const unsigned short*>(P.dO) + (size_t)b * P.ldo + h * DH + 8 * half;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) delta = dot8(delta, __builtin_bit_cast(u32x4_t, of[ks]), *reinterpret_cast<const u32x4_t*>(ug + 16 * ks));
    delta = half_sum(delta);
    if (half == 0 && qrow < Tq) P.delta[(size_t)bh * Tq + qrow] = delta;
    lse2 = (qrow < Tq ? P.LSE[(size_t)bh * Tq + qrow] : 0.f) * LOG2E;
  }
  const float c = a.scale * LOG2E;
  f32x16_t dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = zero16();
  const unsigned tlo = tr_lane_lo(lane), thi = tr_lane_hi(lane);
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  for (int j = 0; j < ntiles; ++j) {
    ring_handover(j, ntiles, issue, [](int) {});
    if constexpr (ACTIVE) {
      const char* sK = smem + (j & 1) * TILE_B;
      const TrBase vaK = tr_base(smem_lds + (j & 1) * TILE_B, tlo, thi);
      const float cc[2] = {ck[0], ck[1]};
      const bf16x8_t one3 = ones3_frag(half == 0);
      if (j + 1 < ntiles) cstat(j + 1);
      auto block = [&](auto KTc) {
        constexpr int KT = decltype(KTc)::value;
        const int k0 = j * 64 + 32 * KT;
        if (k0 >= Tk) return;
        f32x16_t s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        dp = spread_rows(cc[KT], half == 0, one3, s);   // c[key] in every query column
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<DH>(sK, 32 * KT, ks, lane), qf[ks], s, 0, 0, 0);
        constexpr int TD = UNI_TRDEPTH;
        s16x4_t lo[2 * DT], hi[2 * DT];
        DkStepD<DH, KT, TD, 0>::prime(vaK, lo, hi);         // the first K^T fragments land under the dS arithmetic
        const bool ragged = k0 + 32 > Tk;
        f32x16_t ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = fast_exp2(__builtin_fmaf(s[r], c, -lse2));
          const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (ragged) p = key < Tk ? p : 0.f;
          ds[r] = p * (dp[r] - delta);                      // dS^T (scale applied at the store)
        }
        bf16x8_t pf;
        DkStepD<DH, KT, TD, 0>::run(vaK, lo, hi, ds, pf, dq);
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
    }
  }
  if constexpr (ACTIVE) {
    const int lane_e = lane_again();
    store_rows_lds<DH>(dq, a.scale, static_cast<unsigned short*>(P.dQ) + qoff, P.ldq, qs, Tq, lane_e, slice);
  }
}

template <int DH>
__global__ __launch_bounds__(NT, DQ_WAVES_PER_SIMD)
void attn_bwd_dq2u_kernel(const UniArgs u) {
  __shared__ __attribute__((aligned(1024))) char smem[4 * img_tile_bytes<DH>()];
  const AttnArgs2& a = u.a;
  MMF_ATTN_WG_DECODE(a, ROWS_PER_WG, q0);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qs = q0 + 32 * wave;
  if (qs < P.Tq) dq2u_wave<DH, true>(a, P, u.c[pi], bh, qs, smem);
  else           dq2u_wave<DH, false>(a, P, u.c[pi], bh, qs, smem);
}

// One wave of the uniform dK/dV kernel: dkv2_wave without the dP and dV^T chains, the dO tile and the V rows.  dS = p (c_k - delta[q])
// with c_k this lane's key's scalar; w = sum_q p[q][key] is summed per lane over the sweep (the two halves of a wave hold the same key
// for different query rows) and dV[key,:] = w u_h is written as rows.  Query rows past Tq take LSE = +big, so that their p is 0
// (the general kernel lets p = 1 meet dO = 0).  No sweep split: a self-attention with <= 32 keys has one tile to sweep.
template <int DH, bool ACTIVE>
__device__ __forceinline__ void dkv2u_wave(const AttnArgs2& a, const mmf_attn_problem& P, const float* cst, const int bh,
                                           const int k0, char* smem) {
  constexpr int KS = DH / 16, DT = DH / 32, TILE_B = img_tile_bytes<DH>();
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tq = P.Tq, Tk = P.Tk, H = P.H;
  const int b = bh / H, h = bh % H;
  const unsigned short* Qg = static_cast<const unsigned short*>(P.Q) + (size_t)b * Tq * P.ldq + h * DH;
  const __amdgpu_buffer_rsrc_t rsL = f32_rsrc(P.LSE + (size_t)bh * Tq, Tq), rsD = f32_rsrc(P.delta + (size_t)bh * Tq, Tq);
  TileDma<DH> dma;
  dma.init(P.ldq, P.ldq, wave, lane);
  auto issue = [&](int j) { dma.issue_x(Qg + (size_t)64 * j * P.ldq, P.ldq, Tq - 64 * j, smem + (j & 1) * TILE_B, wave); };
  float st_l[2], st_d[2];                                    // ... with LSE = +big for the rows past Tq
  auto stats = [&](int j) { row_stats<true>(rsL, rsD, j, lane, Tq, st_l, st_d); };
  const int ntiles = (Tq + 63) / 64;
  issue(0);
  if constexpr (ACTIVE) stats(0);

  const size_t koff = (size_t)b * Tk * P.ldk + h * DH, voff = (size_t)b * Tk * P.ldv + h * DH;
  char* slice = smem + 2 * TILE_B + wave * img_slice_bytes<DH>();
  bf16x8_t kf[KS];
  float ckey = 0.f;
  if constexpr (ACTIVE) {
    const __amdgpu_buffer_rsrc_t rsC = f32_rsrc(cst + (size_t)bh * Tk, Tk);
    RowLoad<DH> rk;
    rk.issue(rows_rsrc(P.K, koff, Tk, P.ldk), P.ldk, k0, lane);
    ckey = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsC, (unsigned)(k0 + (lane & 31)) * 4u, 0, 0));
    rk.commit(kf, lane, slice);
  }
  f32x16_t dk[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = zero16();
  float w = 0.f;
  const float c = a.scale * LOG2E;
  const unsigned tlo = tr_lane_lo(lane), thi = tr_lane_hi(lane);
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  for (int j = 0; j < ntiles; ++j) {
    ring_handover(j, ntiles, issue, [](int) {});
    if constexpr (ACTIVE) {
      const char* sQ = smem + (j & 1) * TILE_B;
      // this tile's row statistics as MFMA operands; the next tile's are requested now and land under this tile's work
      const float nls = -1.f / a.scale;
      const float cl[2] = {st_l[0] * nls, st_l[1] * nls}, cd[2] = {-st_d[0], -st_d[1]};
      const bf16x8_t one3 = ones3_frag(half == 0);
      if (j + 1 < ntiles) stats(j + 1);
      const TrBase vaQ = tr_base(smem_lds + (j & 1) * TILE_B, tlo, thi);
      auto block = [&](auto QSc) {
        constexpr int QS = decltype(QSc)::value;
        const int q0 = j * 64 + 32 * QS;
        if (q0 >= Tq) return;
        f32x16_t s, dm, z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        s = spread_rows(cl[QS], half == 0, one3, z);    // S' starts at -LSE / scale
        dm = spread_rows(cd[QS], half == 0, one3, z);   // -delta[q] in every key column
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<DH>(sQ, 32 * QS, ks, lane), kf[ks], s, 0, 0, 0);
        constexpr int TD = UNI_TRDEPTH;
        s16x4_t lo[2 * DT], hi[2 * DT];
        DkStepD<DH, QS, TD, 0>::prime(vaQ, lo, hi);         // the first Q^T fragments land under the P / dS arithmetic
        f32x16_t ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fast_exp2(s[r] * c);
          w += p;
          ds[r] = p * (dm[r] + ckey);
        }
        bf16x8_t dsf;
        DkStepD<DH, QS, TD, 0>::run(vaQ, lo, hi, ds, dsf, dk);
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
    }
  }
  if constexpr (ACTIVE) {
    const int lane_e = lane_again();
    store_rows_lds<DH>(dk, a.scale, static_cast<unsigned short*>(P.dK) + koff, P.ldk, k0, Tk, lane_e, slice);
    // dV[key,:] = w u_h in the accumulator layout store_rows_lds takes: register 4g+i of tile dt is column 32 dt + 8 g + 4 half + i
    const float wt = half_sum(w);
    const unsigned short* ug = static_cast<const unsigned short*>(P.dO) + (size_t)b * P.ldo + h * DH + 4 * (lane_e >> 5);
    f32x16_t dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const u32x2_t uu = *reinterpret_cast<const u32x2_t*>(ug + 32 * dt + 8 * g);
        dv[dt][4 * g + 0] = wt * bf16lo(uu[0]); dv[dt][4 * g + 1] = wt * bf16hi(uu[0]);
        dv[dt][4 * g + 2] = wt * bf16lo(uu[1]); dv[dt][4 * g + 3] = wt * bf16hi(uu[1]);
      }
    store_rows_lds<DH>(dv, 1.f, static_cast<unsigned short*>(P.dV) + voff, P.ldv, k0, Tk, lane_e, slice);
  }
}

template <int DH>
__global__ __launch_bounds__(NT, 3)      // dK^T and the K fragments are 72 registers: three waves per SIMD, as the dQ kernels
void attn_bwd_dkv2u_kernel(const UniArgs u) {
  __shared__ __attribute__((aligned(1024))) char smem[4 * img_tile_bytes<DH>()];
  const AttnArgs2& a = u.a;
  MMF_ATTN_WG_DECODE(a, ROWS_PER_WG, kc0);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = kc0 + 32 * wave;
  if (k0 < P.Tk) dkv2u_wave<DH, true>(a, P, u.c[pi], bh, k0, smem);
  else           dkv2u_wave<DH, false>(a, P, u.c[pi], bh, k0, smem);
}

}  // namespace

#ifdef MMF_ATTN_STAMPS
extern "C" int mmf_debug_attn2_stamps(unsigned long long* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_bstamps), &buf, sizeof(buf)) == hipSuccess ? 0 : 1;
}
#endif

// MMF_ATTN_STUBS (build-time, measurement only; tools/build_variant.sh): MMF_ATTN_STUB bits 1 / 2 / 4 skip the forward / dQ / dK/dV
// launches, to read off what the step's time owes to each of them (the outputs are garbage).
#ifdef MMF_ATTN_STUBS
static const int g_attn_stub = [] { const char* e = getenv("MMF_ATTN_STUB"); return e ? atoi(e) : 0; }();
#else
constexpr int g_attn_stub = 0;
#endif

namespace {
// one launch of `total` NT-thread workgroups; the instantiation comes from attn_select (attn_helpers.h)
template <typename K, typename Args>
void launch(K kernel, int total, hipStream_t s, const Args& args) { hipLaunchKernelGGL(kernel, dim3(total), dim3(NT), 0, s, args); }
}  // namespace

int mmf_attn_bwd2_launch(const mmf_attn_problem* problems, int n, int head_dim, float scale, float drop_p,
                         const uint64_t* rng_state, uint32_t site, hipStream_t s, bool given_delta, uint32_t stream_base) {
  if (int rc = check_ranges("mmf_attn_bwd_grouped", problems, n)) return rc;
  AttnArgs2 a;
  if (given_delta || !(g_attn_stub & 2)) {                  // dQ first: from the caller's delta, or writing delta on its way
    const int total = fill_args2(a, problems, n, scale, drop_p, rng_state, site, false, false, stream_base);
    if (given_delta) attn_select(head_dim, a.drop_thresh != 0u, [&](auto dh, auto dr) { launch(attn_bwd_dq2_kernel<dh(), dr(), true>, total, s, a); });
    else             attn_select(head_dim, a.drop_thresh != 0u, [&](auto dh, auto dr) { launch(attn_bwd_dq2_kernel<dh(), dr(), false>, total, s, a); });
    MMF_CHECK_LAUNCH(given_delta ? "mmf_attn_bwd_grouped_delta(dq, v2)" : "mmf_attn_bwd_grouped(dq, v2)");
  }
  if (g_attn_stub & 4) return MMF_OK;
  const int total = fill_args2(a, problems, n, scale, drop_p, rng_state, site, true, false, stream_base);   // then dK/dV (reads delta)
  attn_select(head_dim, a.drop_thresh != 0u, [&](auto dh, auto dr) { launch(attn_bwd_dkv2_kernel<dh(), dr()>, total, s, a); });
  MMF_CHECK_LAUNCH("mmf_attn_bwd_grouped(dkv, v2)");
  return MMF_OK;
}

// Called by mmf_attn_bwd_grouped_uniform (attention.hip) after validation.  cws: the c arrays, problem i's B*H*Tk floats behind
// problem i - 1's (mmf_attn_bwd_grouped_uniform_workspace_bytes).
// dys (may be null): per problem the (B, lddy) pooled gradient the statistics kernel makes dO from (mmf_attn_bwd_grouped_pooled).
int mmf_attn_bwd2u_launch(const mmf_attn_problem* problems, int n, int head_dim, float scale, float* cws, hipStream_t s,
                          const void* const* dys, int lddy) {
  if (int rc = check_ranges("mmf_attn_bwd_grouped_uniform", problems, n)) return rc;
  float* cst[MMF_ATTN_MAX_PROBLEMS];
  StatArgs sa;
  sa.nprob = n;
  int sblocks = 0;
  for (int i = 0; i < n; ++i) {
    const mmf_attn_problem& q = problems[i];
    cst[i] = cws;
    cws += (size_t)q.B * q.H * q.Tk;
    sa.j[i] = {static_cast<const unsigned short*>(q.V), static_cast<const unsigned short*>(q.dO), cst[i], q.B, q.H, q.Tk, q.ldv, q.ldo,
               dys ? static_cast<const unsigned short*>(dys[i]) : nullptr, lddy, 1.f / (float)q.Tq};
    sa.blk_start[i] = sblocks;
    const long long chunks = (long long)q.B * q.Tk * q.H * (head_dim / 8);
    if (chunks > 0x7fffffffLL || (chunks + STAT_CHUNKS - 1) / STAT_CHUNKS + sblocks > 0x7fffffffLL)
      MMF_FAIL(MMF_E_SHAPE, "mmf_attn_bwd_grouped_uniform[%d]: B*Tk*H*head_dim exceeds the statistics launch", i);
    sblocks += (int)((chunks + STAT_CHUNKS - 1) / STAT_CHUNKS);
  }
  sa.blk_start[n] = sblocks;
  attn_select(head_dim, false, [&](auto dh, auto) {
    hipLaunchKernelGGL(attn_uniform_stats_kernel<dh()>, dim3(sblocks), dim3(STAT_THREADS), 0, s, sa);
  });
  MMF_CHECK_LAUNCH("mmf_attn_bwd_grouped_uniform(stats)");
  UniArgs ua;
  auto fill = [&](bool by_keys) {
    const int total = fill_args2(ua.a, problems, n, scale, 0.f, nullptr, 0u, by_keys, false);
    for (int k = 0; k < n; ++k) ua.c[k] = cst[ua.a.orig[k]];
    return total;
  };
  int total = fill(false);
  attn_select(head_dim, false, [&](auto dh, auto) { launch(attn_bwd_dq2u_kernel<dh()>, total, s, ua); });
  MMF_CHECK_LAUNCH("mmf_attn_bwd_grouped_uniform(dq)");
  total = fill(true);
  attn_select(head_dim, false, [&](auto dh, auto) { launch(attn_bwd_dkv2u_kernel<dh()>, total, s, ua); });
  MMF_CHECK_LAUNCH("mmf_attn_bwd_grouped_uniform(dkv)");
  return MMF_OK;
}

// Called by mmf_attn_fwd_grouped_ex (attention.hip) after validation.
int mmf_attn_fwd2_launch(const mmf_attn_problem* problems, int n, int head_dim, float scale, float drop_p,
                         const uint64_t* rng_state, uint32_t site, hipStream_t s, uint32_t stream_base) {
  if (int rc = check_ranges("mmf_attn_fwd_grouped", problems, n)) return rc;
  if (g_attn_stub & 1) return MMF_OK;
  AttnArgs2 a;
  const int total = fill_args2(a, problems, n, scale, drop_p, rng_state, site, false, true, stream_base);
  attn_select(head_dim, a.drop_thresh != 0u, [&](auto dh, auto dr) { launch(attn_fwd2n_kernel<dh(), dr()>, total, s, a); });
  MMF_CHECK_LAUNCH("mmf_attn_fwd_grouped");
  return MMF_OK;
}
