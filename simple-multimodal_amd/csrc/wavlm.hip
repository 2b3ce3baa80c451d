// WavLM's gated relative position bias (HuggingFace WavLMAttention): the gate, and the fused attention forward that adds
//     score[b,h,i,j] = scale q_i . k_j + g[b,h,i] * tab[h][j - i + T - 1]
// without ever forming a (T, T) bias.  Self-attention only (Tq == Tk = T).
//
// mmf_wavlm_gate (streaming): the 8-output linear every head shares, on the head's slice of the layer INPUT row, then
//     g = sigmoid(a) (sigmoid(b) const_h - 1) + 2,   a = sum of outputs 0..3, b = of outputs 4..7
// One 16-byte chunk of a row per lane (fully coalesced, as attn_uniform_stats_kernel reads V), the chunk's eight partial dot products
// into LDS, then one thread per (row, head) adds the head's DH/8 partial sums in chunk order: f32, fixed order, no atomics.
//
// mmf_attn_fwd_relbias: the plain forward's wave body (attention2.hip fwd2_wave: S^T = K.Q^T with the query on the lane, online softmax
// with the deferred maximum, O^T += V^T.P^T from the accumulator, 2-stage LDS-DMA ring) with one more term.  In that orientation the
// gate is a per-lane scalar and a lane's 16 accumulator rows of a 32-key block are four runs of four consecutive keys, so the lane
// needs four runs of four consecutive table entries: tab[h][k0 + 8 g + 4 half - i + T - 1 ..+3], g = 0..3.  They are read straight
// from the table (2T - 1 floats per head: it stays in L2 / the vector cache, and neighbouring lanes read overlapping windows), NOT
// staged in LDS: the LDS port is as busy as the matrix pipe in these kernels, and the runs start at any dword, which a ds_read_b128
// cannot.  Per tile a wave issues its eight 16-byte reads (both blocks) right behind the ring's barrier and AHEAD of the next tile's
// LDS-DMA, so the counted wait in front of their first use leaves that DMA in flight (vmcnt returns in order); the last tile, which
// issues no DMA, is a second instantiation of the tile body rather than a branch in it, because a branch merges the two wait counts
// to the stricter one.  Blocks at the edge (keys past T in the block, or query rows past T in the wave) take sixteen 4-byte reads at
// clamped indices instead: every index a live (query, key) pair forms is in 0 .. 2T - 2 by construction, the clamp only moves what
// masked keys and dead rows read.  The bias enters as s += (g / scale) tab on the raw scores, so the softmax that follows is the
// plain kernel's to the instruction, and LSE is that of the biased scores (what a backward needs).
#include "attn2_common.h"

namespace {

// ---- the gate ---------------------------------------------------------------------------------------------------------
constexpr int GATE_THREADS = 256, GATE_PASSES = 3, GATE_CHUNKS = GATE_THREADS * GATE_PASSES;     // 768 = 96 heads of 8 chunks = 64 of 12

template <int DH>
__global__ __launch_bounds__(GATE_THREADS)
void wavlm_gate_kernel(const unsigned short* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ bias,
                       const float* __restrict__ cst, float* __restrict__ gate, int n, int T, int H) {
  constexpr int CPH = DH / 8, NG = GATE_CHUNKS / CPH;
  static_assert(GATE_CHUNKS % CPH == 0, "a head's chunks must not straddle two workgroups");
  __shared__ __attribute__((aligned(16))) float sw[8 * DH];
  __shared__ float part[8][GATE_CHUNKS];
  for (int i = threadIdx.x; i < 8 * DH; i += GATE_THREADS) sw[i] = w[i];
  __syncthreads();
  const unsigned cpr = (unsigned)(H * CPH), nchunks = (unsigned)(n * T) * cpr;              // (the host checked the range)
#pragma unroll
  for (int i = 0; i < GATE_PASSES; ++i) {
    const unsigned slot = threadIdx.x + GATE_THREADS * i, idx = blockIdx.x * GATE_CHUNKS + slot;
    if (idx < nchunks) {
      const unsigned row = idx / cpr, ch = idx - row * cpr, c = ch % CPH;
      float xf[8];
      unpack8(*reinterpret_cast<const u32x4_t*>(x + (size_t)row * ldx + ch * 8), xf);
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const float4 w0 = ld4(sw + o * DH + c * 8), w1 = ld4(sw + o * DH + c * 8 + 4);
        float s = xf[0] * w0.x;
        s = fmaf(xf[1], w0.y, s); s = fmaf(xf[2], w0.z, s); s = fmaf(xf[3], w0.w, s);
        s = fmaf(xf[4], w1.x, s); s = fmaf(xf[5], w1.y, s); s = fmaf(xf[6], w1.z, s); s = fmaf(xf[7], w1.w, s);
        part[o][slot] = s;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < NG) {
    const unsigned pair = blockIdx.x * NG + threadIdx.x;       // (row, head)
    if (pair < (unsigned)(n * T * H)) {
      float v[8];
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        float s = part[o][threadIdx.x * CPH];
#pragma unroll
        for (int e = 1; e < CPH; ++e) s += part[o][threadIdx.x * CPH + e];
        v[o] = s + bias[o];
      }
      const float a = ((v[0] + v[1]) + v[2]) + v[3], b = ((v[4] + v[5]) + v[6]) + v[7];
      const float sa = 1.f / (1.f + expf(-a)), sb = 1.f / (1.f + expf(-b));
      const unsigned row = pair / (unsigned)H, h = pair - row * H, bi = row / (unsigned)T, t = row - bi * T;
      gate[((size_t)bi * H + h) * T + t] = sa * (sb * cst[h] - 1.f) + 2.f;
    }
  }
}

// ---- the attention forward ----------------------------------------------------------------------------------------------
struct RelArgs {
  mmf_attn_problem p;
  float scale;
  int nwg, nchunk, rpc, n8;               // real workgroups = B*H*nchunk; rows per chunk; padded grid / 8 (the XCD map of work_item)
  const float* gate;                      // (B, H, T)
  const float* tab;                       // (H, 2T - 1)
};

// One wave: its 32-row query block at rows qs (ACTIVE), or staging and barriers only.  fwd2_wave's text with the bias term.
template <int DH, bool ACTIVE>
__device__ __forceinline__ void relbias_wave(const RelArgs& a, const int bh, const int qs, char* smem) {
  constexpr int KS = DH / 16, DT = DH / 32, TILE_B = img_tile_bytes<DH>(), STAGE_B = 2 * TILE_B;
  const mmf_attn_problem& P = a.p;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = P.Tq, H = P.H;
  const int b = bh / H, h = bh % H;

  const unsigned short* Kg = static_cast<const unsigned short*>(P.K) + (size_t)b * T * P.ldk + h * DH;
  const unsigned short* Vg = static_cast<const unsigned short*>(P.V) + (size_t)b * T * P.ldv + h * DH;
  TileDma<DH> dma;
  dma.init(P.ldk, P.ldv, wave, lane);
  auto issue = [&](int j) {
    dma.issue(Kg + (size_t)64 * j * P.ldk, Vg + (size_t)64 * j * P.ldv, P.ldk, P.ldv, T - 64 * j, smem + (j & 1) * STAGE_B, wave);
  };
  const int ntiles = (T + 63) / 64;
  issue(0);

  char* slice = smem + STAGE_B + wave * img_slice_bytes<DH>();
  bf16x8_t qf[KS];
  const int qi = qs + (lane & 31);
  float gs = 0.f;                                            // g / scale: the bias joins the RAW scores
  if constexpr (ACTIVE) {
    const unsigned short* Qg = static_cast<const unsigned short*>(P.Q) + (size_t)b * T * P.ldq + h * DH;
    RowLoad<DH> rl;
    rl.issue(rows_rsrc(Qg, 0, T, P.ldq), P.ldq, qs, lane);
    if (qi < T) gs = a.gate[(size_t)bh * T + qi] / a.scale;
    rl.commit(qf, lane, slice);
  }
  // tab[h][key - qi + T - 1]: this lane's index of key 0 of its first run; block k0, run g, element e add k0 + 8 g + e
  const int nt = 2 * T - 1, tb0 = T - 1 - qi + 4 * half;
  const __amdgpu_buffer_rsrc_t rsT = f32_rsrc(a.tab + (size_t)h * nt, nt);
  const bool qfull = qs + 32 <= T;                           // wave-uniform: every lane's query row exists

  f32x16_t o[DT];
  float m = NEG_BIG, l = 0.f;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = zero16();
  const float c = a.scale * LOG2E;
  const unsigned tlo = tr_lane_lo(lane), thi = tr_lane_hi(lane);
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // tile j; LAST: the tile that issues no DMA behind it (a second instantiation, see the head of the file)
  auto tile = [&](const int j, auto LASTc) {
    constexpr bool LAST = decltype(LASTc)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the ring hand-over (ring_handover, attn2_common.h) ...
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int kb = j * 64;
    f32x4_t tb[2][4];                                        // ... with this tile's table runs requested ahead of the next tile's DMA
    if constexpr (ACTIVE) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const int k0 = kb + 32 * kt;
        if (k0 >= T) continue;
        if (qfull && k0 + 32 <= T) {                         // wave-uniform: every index of the block is in 0 .. 2T - 2
#pragma unroll
          for (int g = 0; g < 4; ++g)
            tb[kt][g] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rsT, (unsigned)(tb0 + k0 + 8 * g) * 4u, 0, 0));
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int ix = min(max(tb0 + k0 + 8 * g + e, 0), nt - 1);
              tb[kt][g][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsT, (unsigned)ix * 4u, 0, 0));
            }
        }
      }
    }
    if constexpr (!LAST) issue(j + 1);
    if constexpr (ACTIVE) {
      const char* sK = smem + (j & 1) * STAGE_B;
      const TrBase vaV = tr_base(smem_lds + (j & 1) * STAGE_B + TILE_B, tlo, thi);
      auto block = [&](auto KTc) {
        constexpr int KT = decltype(KTc)::value;
        const int k0 = kb + 32 * KT;
        if (k0 >= T) return;                               // wave-uniform: nothing but masked keys
        f32x16_t s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        bf16x8_t kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = row_frag<DH>(sK, 32 * KT, ks, lane);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);                 // the asm V^T reads below are invisible to the compiler's lgkmcnt count
        constexpr int TD = FWD_TRDEPTH;
        s16x4_t lo[2 * DT], hi[2 * DT];
        PvStepD<DH, KT, TD, 0>::prime(vaV, lo, hi);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_fmaf(tb[KT][r >> 2][r & 3], gs, s[r]);     // + g bias / scale
        if (k0 + 32 > T) {                                 // ragged block
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            s[r] = key < T ? s[r] : NEG_BIG;
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
        bf16x8_t pf;
        PvStepD<DH, KT, TD, 0>::run(vaV, lo, hi, s, pf, o);
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
    }
  };
  for (int j = 0; j + 1 < ntiles; ++j) tile(j, std::false_type{});
  tile(ntiles - 1, std::true_type{});

  if constexpr (ACTIVE) {
    // the stage the last tile did not use is free (every wave passed the last barrier): reuse the wave's slice there
    char* oslice = smem + (ntiles & 1) * STAGE_B + wave * img_slice_bytes<DH>();
    unsigned short* Og = static_cast<unsigned short*>(P.O) + (size_t)b * T * P.ldo + h * DH;
    const float lt = half_sum(l);
    const int lane_e = lane_again();
    store_rows_lds<DH>(o, 1.f / lt, Og, P.ldo, qs, T, lane_e, oslice);
    const int qrow = qs + (lane & 31);
    if (half == 0 && qrow < T) P.LSE[(size_t)bh * T + qrow] = m * LN2 + __logf(lt);
  }
}

// The plain forward's workgroup: one 32-row query block per wave, three workgroups per CU (attn_fwd2n_kernel, attention2.hip)
template <int DH>
__global__ __launch_bounds__(NT, 3)
void attn_fwd_relbias_kernel(const RelArgs a) {
  constexpr int STAGE_B = 2 * img_tile_bytes<DH>();
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];
  const int bid = blockIdx.x, item = (bid & 7) * a.n8 + (bid >> 3);      // XCD x walks a contiguous range of the work items
  if (item >= a.nwg) return;
  const int bh = item / a.nchunk, q0 = (item % a.nchunk) * a.rpc;
  const int nb = (min(a.p.Tq, q0 + a.rpc) - q0 + 31) >> 5;               // 32-row query blocks in this chunk (1..4)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qs = q0 + 32 * wave;
  if (wave < nb) relbias_wave<DH, true>(a, bh, qs, smem);
  else           relbias_wave<DH, false>(a, bh, qs, smem);
}

}  // namespace

extern "C" int mmf_wavlm_gate(const void* x_bf16, int ldx, const float* lin_w, const float* lin_b, const float* head_const,
                              float* gate, int n, int T, int H, int head_dim, void* stream) {
  const char* fn = "mmf_wavlm_gate";
  if (!x_bf16 || !lin_w || !lin_b || !head_const || !gate) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", fn);
  if (head_dim != 64 && head_dim != 96) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: head_dim=%d (supported: 64, 96)", fn, head_dim);
  if (n <= 0 || T <= 0 || H <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: n=%d T=%d H=%d", fn, n, T, H);
  const long long chunks = (long long)n * T * H * (head_dim / 8);
  if (chunks > 0x7fffffffLL)
    MMF_FAIL(MMF_E_SHAPE, "%s: n*T*H*head_dim exceeds the launch", fn);
  if (ldx < H * head_dim || (ldx & 7) || !mmf_aligned16(x_bf16) || !mmf_aligned16(lin_w))
    MMF_FAIL(MMF_E_ALIGN, "%s: x and the linear's weight must be 16-byte aligned, ldx >= H*head_dim and a multiple of 8", fn);
  if ((reinterpret_cast<uintptr_t>(lin_b) | reinterpret_cast<uintptr_t>(head_const) | reinterpret_cast<uintptr_t>(gate)) & 3u)
    MMF_FAIL(MMF_E_ALIGN, "%s: bias, constant and gate must be 4-byte aligned", fn);
  const int blocks = (int)((chunks + GATE_CHUNKS - 1) / GATE_CHUNKS);
  attn_select(head_dim, false, [&](auto dh, auto) {
    hipLaunchKernelGGL(wavlm_gate_kernel<dh()>, dim3(blocks), dim3(GATE_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned short*>(x_bf16), ldx, lin_w, lin_b, head_const, gate, n, T, H);
  });
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_attn_fwd_relbias(const mmf_attn_problem* problem, int head_dim, float scale, const float* gate,
                                    const float* table, void* stream) {
  const char* fn = "mmf_attn_fwd_relbias";
  if (!problem) MMF_FAIL(MMF_E_SHAPE, "%s: null problem", fn);
  const mmf_attn_problem& q = *problem;
  if (head_dim != 64 && head_dim != 96) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: head_dim=%d (supported: 64, 96)", fn, head_dim);
  if (q.B <= 0 || q.H <= 0 || q.Tq <= 0 || q.Tk <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: B=%d H=%d Tq=%d Tk=%d", fn, q.B, q.H, q.Tq, q.Tk);
  if (q.Tq != q.Tk) MMF_FAIL(MMF_E_SHAPE, "%s: self-attention only, Tq=%d != Tk=%d", fn, q.Tq, q.Tk);
  if (!q.Q || !q.K || !q.V || !q.O || !q.LSE || !gate || !table) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", fn);
  const int w = q.H * head_dim;
  if (q.ldq < w || q.ldk < w || q.ldv < w || q.ldo < w || (q.ldq & 7) || (q.ldk & 7) || (q.ldv & 7) || (q.ldo & 7))
    MMF_FAIL(MMF_E_ALIGN, "%s: row strides must be >= H*head_dim and multiples of 8", fn);
  if (!mmf_aligned16(q.Q) || !mmf_aligned16(q.K) || !mmf_aligned16(q.V) || !mmf_aligned16(q.O))
    MMF_FAIL(MMF_E_ALIGN, "%s: Q/K/V/O must be 16-byte aligned", fn);
  if ((reinterpret_cast<uintptr_t>(q.LSE) | reinterpret_cast<uintptr_t>(gate) | reinterpret_cast<uintptr_t>(table)) & 3u)
    MMF_FAIL(MMF_E_ALIGN, "%s: LSE, gate and table must be 4-byte aligned", fn);
  if (int rc = check_ranges(fn, problem, 1)) return rc;
  RelArgs a;
  a.p = q; a.scale = scale; a.gate = gate; a.tab = table;
  a.nchunk = (q.Tq + ROWS_PER_WG - 1) / ROWS_PER_WG;
  a.rpc = (((q.Tq + a.nchunk - 1) / a.nchunk) + 31) / 32 * 32;          // the chunks of a (b, h) balanced, as the plain forward's
  const long long nwg = (long long)q.B * q.H * a.nchunk;
  if (nwg > 0x7ffffff0LL) MMF_FAIL(MMF_E_SHAPE, "%s: B*H*chunks exceeds the launch", fn);
  a.nwg = (int)nwg;
  a.n8 = (a.nwg + 7) / 8;
  attn_select(head_dim, false, [&](auto dh, auto) {
    hipLaunchKernelGGL(attn_fwd_relbias_kernel<dh()>, dim3(8 * a.n8), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
  });
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}
