// The BERT family's two own pieces (HuggingFace BertModel / RobertaModel, absolute positions): the embedding row, and the plain fused
// attention forward with a key padding mask.  Self-attention only (Tq == Tk = T).
//
// mmf_bert_embed (one wave per row, the form of deberta_embed_kernel): out[r] = bf16(LayerNorm((word[ids[r]] | embeds[r]) +
// type[tt[r]] + pos[p(r)])) on f32 rows, the sum in HuggingFace's order, carried in f64 inside the wave (see the kernel).  p(r)
// for token t of its item: t (BERT); RoBERTa on the ids route
// pad + #{ids != pad among tokens 0 .. t} where ids[r] != pad and pad otherwise, the count formed by the wave itself from coalesced
// loads of the item's ids, a ballot and a popcount per 64 ids; RoBERTa on the embeds route pad + 1 + t.  Ids, type ids and positions
// are clamped into their tables.
//
// mmf_mask_pack (one workgroup per item): an (n, T) mask (kind 0 none, 1 f32, 2 u8) -> per item a row of 2 + 2 ceil(T / 64) 32-bit
// words: [0] one past the last valid key, [1] the count of valid keys, [2 + w] bit k = key 32 w + k is valid (keys past T: 0; the
// row is padded to whole 64-key tiles so that a tile's two words are one aligned 8-byte read).  One launch, no host step.
//
// mmf_attn_fwd_keymask: the plain forward's wave body (attention2.hip fwd2_wave, as relbias_wave of wavlm.hip restates it: S^T =
// K.Q^T with the query on the lane, online softmax with the deferred maximum, O^T += V^T.P^T from the accumulator, 2-stage LDS-DMA
// ring) reading that row.  In this orientation a lane's 16 accumulator rows are 16 KEYS of the 32-key block and every lane of the
// wave sees the same 32 keys, so a block's mask is one wave-uniform word: a word of all ones costs nothing beyond its compare, a
// word of 0 skips the block (no K fragment reads, no MFMAs), anything else sends the masked keys down the NEG_BIG path that ragged
// keys past T take in the plain kernel (their bits are 0 too, so this select IS the ragged select).  The tile loop ends at
// ceil(last / 64): tiles past the last valid key are never staged.  Only keys are masked: every query row 0 .. T - 1 is computed.
// An item without a valid key is the uniform row over all T keys (what score + finfo.min gives in f32): a wave-uniform flag walks
// all tiles with every score 0, so O is the mean of the T value rows and LSE = ln T.  Since a block with a non-zero word has a valid
// key for every query row, the running maximum is a real score from the first block a wave computes, and nothing is NaN or Inf.
#include "attn2_common.h"

namespace {

// ---- the embedding row -----------------------------------------------------------------------------------------------
constexpr int BE_THREADS = 256;
constexpr int POS_BERT = 0, POS_ROBERTA = 1;

__device__ __forceinline__ long long be_clamp(long long x, int n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

__device__ __forceinline__ double be_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(BE_THREADS)
void bert_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ embeds, const long long* __restrict__ types,
                       const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
                       const float* __restrict__ gamma, const float* __restrict__ beta, unsigned short* __restrict__ out, int rows,
                       int T, int d, int vocab, int npos, int ntype, int rule, long long pad, float eps) {
  const int row = blockIdx.x * (BE_THREADS / MMF_WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int item = row / T, t = row - item * T;
  long long p = t;
  if (rule == POS_ROBERTA) {
    if (ids) {
      const long long* __restrict__ it = ids + (size_t)item * T;
      int count = 0;
      for (int q0 = 0; q0 <= t; q0 += MMF_WAVE) {            // (wave-uniform trip count)
        const int q = q0 + lane;
        count += __popcll(__ballot(q <= t && it[q] != pad));
      }
      p = it[t] != pad ? pad + count : pad;
    } else {
      p = pad + 1 + t;
    }
  }
  const float* __restrict__ src = ids ? word + (size_t)be_clamp(ids[row], vocab) * d : embeds + (size_t)row * d;
  const float* __restrict__ tr = type + (size_t)be_clamp(types ? types[row] : 0, ntype) * d;
  const float* __restrict__ pr = pos + (size_t)be_clamp(p, npos) * d;
  // lane l owns columns 4 l + 256 k (k < 4, so d <= 1024): mean, then the centred second moment, as torch's LayerNorm.  The sum
  // of the three rows, the statistics and the normalisation are carried in f64: an output that falls next to zero is the
  // difference of O(1) terms, and in f32 its error is many bf16 spacings OF THAT OUTPUT (torch's own f32 LayerNorm is three off
  // at such an element).  In f64 every element is the float64 LayerNorm rounded once, whatever its size; the kernel is bound by
  // its row reads, the 4 d f64 operations of a row are not what it waits for.
  double v[4][4];
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * lane + 256 * k;
    f32x4_t w = {0.f, 0.f, 0.f, 0.f}, ty = w, q = w;
    if (c < d) {
      w = *reinterpret_cast<const f32x4_t*>(src + c);
      ty = *reinterpret_cast<const f32x4_t*>(tr + c);
      q = *reinterpret_cast<const f32x4_t*>(pr + c);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[k][e] = ((double)w[e] + (double)ty[e]) + (double)q[e];
    sum += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  }
  const double mean = be_wave_sum(sum) / (double)d;
  double sq = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (4 * lane + 256 * k < d) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const double c = v[k][e] - mean; sq = fma(c, c, sq); }
    }
  }
  const double rstd = 1.0 / sqrt(be_wave_sum(sq) / (double)d + (double)eps);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < d) {
      const f32x4_t g = *reinterpret_cast<const f32x4_t*>(gamma + c), b = *reinterpret_cast<const f32x4_t*>(beta + c);
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = (float)fma((v[k][e] - mean) * rstd, (double)g[e], (double)b[e]);
      *reinterpret_cast<u32x2_t*>(out + (size_t)row * d + c) = u32x2_t{pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3])};
    }
  }
}

// ---- the packed mask ---------------------------------------------------------------------------------------------------
constexpr int MP_THREADS = 256, MP_WAVES = MP_THREADS / MMF_WAVE;

__device__ __forceinline__ bool mp_valid(const void* __restrict__ mask, int kind, size_t i) {
  if (kind == 1) return static_cast<const float*>(mask)[i] != 0.0f;
  if (kind == 2) return static_cast<const unsigned char*>(mask)[i] != 0;
  return true;
}

__host__ __device__ constexpr int mp_row_words(int T) { return 2 + 2 * ((T + 63) / 64); }

__global__ __launch_bounds__(MP_THREADS)
void mask_pack_kernel(const void* __restrict__ mask, int kind, unsigned* __restrict__ packed, int T) {
  __shared__ int s_last[MP_WAVES], s_count[MP_WAVES];
  const int item = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned* __restrict__ row = packed + (size_t)item * mp_row_words(T);
  int last = 0, count = 0;
  for (int j = wave; 64 * j < T; j += MP_WAVES) {            // (wave-uniform) one 64-key tile per step
    const int key = 64 * j + lane;
    const unsigned long long bits = __ballot(key < T && mp_valid(mask, kind, (size_t)item * T + key));
    if (lane == 0) { row[2 + 2 * j] = (unsigned)bits; row[3 + 2 * j] = (unsigned)(bits >> 32); }
    count += __popcll(bits);
    if (bits) last = 64 * j + 64 - __clzll((long long)bits);
  }
  if (lane == 0) { s_last[wave] = last; s_count[wave] = count; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < MP_WAVES; ++w) { last = max(last, s_last[w]); count += s_count[w]; }
    row[0] = (unsigned)last;
    row[1] = (unsigned)count;
  }
}

// ---- the attention forward ----------------------------------------------------------------------------------------------
struct KeyArgs {
  mmf_attn_problem p;
  float scale;
  int nwg, nchunk, rpc, n8;               // real workgroups = B*H*nchunk; rows per chunk; padded grid / 8 (the XCD map of work_item)
  const unsigned* packed;                 // (B, mp_row_words(T)): mask_pack_kernel's rows
};

// One wave: its 32-row query block at rows qs (ACTIVE), or staging and barriers only.  fwd2_wave's text with the key mask.
template <int DH, bool ACTIVE>
__device__ __forceinline__ void keymask_wave(const KeyArgs& a, const int bh, const int qs, char* smem) {
  constexpr int KS = DH / 16, DT = DH / 32, TILE_B = img_tile_bytes<DH>(), STAGE_B = 2 * TILE_B;
  const mmf_attn_problem& P = a.p;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = P.Tq, H = P.H;
  const int b = bh / H, h = bh % H;

  // the item's mask row: wave-uniform, every word of it
  const unsigned* __restrict__ mrow = a.packed + (size_t)b * mp_row_words(T);
  const int nvalid = __builtin_amdgcn_readfirstlane((int)mrow[1]);
  const bool empty = nvalid <= 0;                            // no valid key: the uniform row over all T keys
  const int last = empty ? T : min(__builtin_amdgcn_readfirstlane((int)mrow[0]), T);
  const int ntiles = max((last + 63) / 64, 1);               // tiles past the last valid key are never staged
  const unsigned long long* __restrict__ mtile = reinterpret_cast<const unsigned long long*>(mrow + 2);

  const unsigned short* Kg = static_cast<const unsigned short*>(P.K) + (size_t)b * T * P.ldk + h * DH;
  const unsigned short* Vg = static_cast<const unsigned short*>(P.V) + (size_t)b * T * P.ldv + h * DH;
  TileDma<DH> dma;
  dma.init(P.ldk, P.ldv, wave, lane);
  auto issue = [&](int j) {
    dma.issue(Kg + (size_t)64 * j * P.ldk, Vg + (size_t)64 * j * P.ldv, P.ldk, P.ldv, T - 64 * j, smem + (j & 1) * STAGE_B, wave);
  };
  issue(0);

  char* slice = smem + STAGE_B + wave * img_slice_bytes<DH>();
  bf16x8_t qf[KS];
  if constexpr (ACTIVE) {
    const unsigned short* Qg = static_cast<const unsigned short*>(P.Q) + (size_t)b * T * P.ldq + h * DH;
    RowLoad<DH> rl;
    rl.issue(rows_rsrc(Qg, 0, T, P.ldq), P.ldq, qs, lane);
    rl.commit(qf, lane, slice);
  }

  f32x16_t o[DT];
  float m = NEG_BIG, l = 0.f;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = zero16();
  const float c = a.scale * LOG2E;
  const unsigned tlo = tr_lane_lo(lane), thi = tr_lane_hi(lane);
  const unsigned smem_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // A tile's 64 mask bits are requested one tile ahead, behind the ring's barrier and AHEAD of the next tile's LDS-DMA (the read
  // comes out as a vector load): its counted wait, at the end of this tile's work, leaves that DMA in flight (vmcnt returns in
  // order), and its latency lies under the tile.  So the hand-over is ring_handover's text with the read in it.
  unsigned long long bits_next = mtile[0];
  for (int j = 0; j < ntiles; ++j) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const unsigned long long bits_now = bits_next;
    if (j + 1 < ntiles) {
      bits_next = mtile[j + 1];
      asm volatile("" ::: "memory");
      issue(j + 1);
    }
    unsigned long long bits64 = bits_now;
    if constexpr (ACTIVE) {
      // keys past T have bit 0; the empty item takes every key below T instead
      if (empty) bits64 = T - 64 * j >= 64 ? ~0ull : (1ull << (T - 64 * j)) - 1ull;
      const unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)bits64), whi = __builtin_amdgcn_readfirstlane((unsigned)(bits64 >> 32));
      const char* sK = smem + (j & 1) * STAGE_B;
      const TrBase vaV = tr_base(smem_lds + (j & 1) * STAGE_B + TILE_B, tlo, thi);
      auto block = [&](auto KTc) {
        constexpr int KT = decltype(KTc)::value;
        const unsigned word = KT ? whi : wlo;
        if (word == 0u) return;                              // wave-uniform: nothing but masked keys
        f32x16_t s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        bf16x8_t kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = row_frag<DH>(sK, 32 * KT, ks, lane);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], s, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);                   // the asm V^T reads below are invisible to the compiler's lgkmcnt count
        constexpr int TD = FWD_TRDEPTH;
        s16x4_t lo[2 * DT], hi[2 * DT];
        PvStepD<DH, KT, TD, 0>::prime(vaV, lo, hi);
        if (empty) {                                         // wave-uniform: all scores 0
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = 0.f;
        }
        if (word != 0xffffffffu) {                           // wave-uniform: a block with masked (or ragged) keys
          const unsigned mine = word >> (4 * half);          // this lane's key of register r: (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = (mine >> ((r & 3) + 8 * (r >> 2))) & 1u ? s[r] : NEG_BIG;
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = half_max(mx) * c;
        if (!__all(mx <= m + DEFER)) {                       // wave-uniform: raise the running maximum
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
  }

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
void attn_fwd_keymask_kernel(const KeyArgs a) {
  constexpr int STAGE_B = 2 * img_tile_bytes<DH>();
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];
  const int bid = blockIdx.x, item = (bid & 7) * a.n8 + (bid >> 3);      // XCD x walks a contiguous range of the work items
  if (item >= a.nwg) return;
  const int bh = item / a.nchunk, q0 = (item % a.nchunk) * a.rpc;
  const int nb = (min(a.p.Tq, q0 + a.rpc) - q0 + 31) >> 5;               // 32-row query blocks in this chunk (1..4)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qs = q0 + 32 * wave;
  if (wave < nb) keymask_wave<DH, true>(a, bh, qs, smem);
  else           keymask_wave<DH, false>(a, bh, qs, smem);
}

}  // namespace

extern "C" int mmf_bert_embed(const int64_t* ids, const float* embeds, const int64_t* token_type_ids, const float* word,
                              const float* pos, const float* type, const float* gamma, const float* beta, float eps, int position_rule,
                              int64_t pad, void* out_bf16, int64_t rows, int T, int d, int vocab, int npos, int ntype, void* stream) {
  const char* fn = "mmf_bert_embed";
  if ((ids == nullptr) == (embeds == nullptr)) MMF_FAIL(MMF_E_SHAPE, "%s: exactly one of ids / embeds", fn);
  if (!pos || !type || !gamma || !beta || !out_bf16 || (ids && !word) || rows <= 0 || T <= 0 || d <= 0 || (ids && vocab <= 0) ||
      npos <= 0 || ntype <= 0 || rows % T)
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or rows=%lld T=%d d=%d vocab=%d positions=%d types=%d (rows a multiple of T)", fn,
             (long long)rows, T, d, vocab, npos, ntype);
  if (position_rule != POS_BERT && position_rule != POS_ROBERTA)
    MMF_FAIL(MMF_E_SHAPE, "%s: position_rule=%d (0 BERT, 1 RoBERTa)", fn, position_rule);
  if ((d & 3) || d > 1024 || rows > ((int64_t)1 << 31) - 4)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: d=%d (multiple of 4, at most 1024), rows=%lld (below 2^31)", fn, d, (long long)rows);
  if (!mmf_aligned16(pos) || !mmf_aligned16(type) || !mmf_aligned16(gamma) || !mmf_aligned16(beta) || !mmf_aligned16(out_bf16) ||
      (ids && !mmf_aligned16(word)) || (embeds && !mmf_aligned16(embeds)) ||
      ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(token_type_ids)) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "%s: tables / embeds / gamma / beta / out must be 16-byte aligned, ids and type ids 8-byte aligned", fn);
  const int per = BE_THREADS / MMF_WAVE;
  hipLaunchKernelGGL(bert_embed_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(BE_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(ids), embeds, reinterpret_cast<const long long*>(token_type_ids), word, pos, type,
                     gamma, beta, static_cast<unsigned short*>(out_bf16), (int)rows, T, d, vocab, npos, ntype, position_rule,
                     (long long)pad, eps);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_mask_pack_words(int T) { return T > 0 ? mp_row_words(T) : 0; }

extern "C" int mmf_mask_pack(const void* mask, int mask_kind, uint32_t* packed, int n, int T, void* stream) {
  const char* fn = "mmf_mask_pack";
  if (mask_kind < 0 || mask_kind > 2 || (mask_kind == 0) != (mask == nullptr))
    MMF_FAIL(MMF_E_SHAPE, "%s: mask_kind=%d (0 none, 1 f32, 2 u8) does not match the mask pointer", fn, mask_kind);
  if (!packed || n <= 0 || T <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: null output or n=%d T=%d", fn, n, T);
  if ((long long)n * T > 0x7fffffffLL) MMF_FAIL(MMF_E_SHAPE, "%s: n*T exceeds the launch", fn);
  if ((mask_kind == 1 && (reinterpret_cast<uintptr_t>(mask) & 3u)) || (reinterpret_cast<uintptr_t>(packed) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "%s: an f32 mask must be 4-byte aligned, the packed rows 8-byte aligned", fn);
  hipLaunchKernelGGL(mask_pack_kernel, dim3(n), dim3(MP_THREADS), 0, static_cast<hipStream_t>(stream), mask, mask_kind, packed, T);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_attn_fwd_keymask(const mmf_attn_problem* problem, int head_dim, float scale, const uint32_t* packed_mask,
                                    void* stream) {
  const char* fn = "mmf_attn_fwd_keymask";
  if (!problem) MMF_FAIL(MMF_E_SHAPE, "%s: null problem", fn);
  const mmf_attn_problem& q = *problem;
  if (head_dim != 64 && head_dim != 96) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: head_dim=%d (supported: 64, 96)", fn, head_dim);
  if (q.B <= 0 || q.H <= 0 || q.Tq <= 0 || q.Tk <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: B=%d H=%d Tq=%d Tk=%d", fn, q.B, q.H, q.Tq, q.Tk);
  if (q.Tq != q.Tk) MMF_FAIL(MMF_E_SHAPE, "%s: self-attention only, Tq=%d != Tk=%d", fn, q.Tq, q.Tk);
  if (!q.Q || !q.K || !q.V || !q.O || !q.LSE || !packed_mask) MMF_FAIL(MMF_E_SHAPE, "%s: null operand", fn);
  const int w = q.H * head_dim;
  if (q.ldq < w || q.ldk < w || q.ldv < w || q.ldo < w || (q.ldq & 7) || (q.ldk & 7) || (q.ldv & 7) || (q.ldo & 7))
    MMF_FAIL(MMF_E_ALIGN, "%s: row strides must be >= H*head_dim and multiples of 8", fn);
  if (!mmf_aligned16(q.Q) || !mmf_aligned16(q.K) || !mmf_aligned16(q.V) || !mmf_aligned16(q.O))
    MMF_FAIL(MMF_E_ALIGN, "%s: Q/K/V/O must be 16-byte aligned", fn);
  if ((reinterpret_cast<uintptr_t>(q.LSE) & 3u) || (reinterpret_cast<uintptr_t>(packed_mask) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "%s: LSE must be 4-byte aligned, the packed mask 8-byte aligned", fn);
  if (int rc = check_ranges(fn, problem, 1)) return rc;
  KeyArgs a;
  a.p = q; a.scale = scale; a.packed = packed_mask;
  a.nchunk = (q.Tq + ROWS_PER_WG - 1) / ROWS_PER_WG;
  a.rpc = (((q.Tq + a.nchunk - 1) / a.nchunk) + 31) / 32 * 32;          // the chunks of a (b, h) balanced, as the plain forward's
  const long long nwg = (long long)q.B * q.H * a.nchunk;
  if (nwg > 0x7ffffff0LL) MMF_FAIL(MMF_E_SHAPE, "%s: B*H*chunks exceeds the launch", fn);
  a.nwg = (int)nwg;
  a.n8 = (a.nwg + 7) / 8;
  attn_select(head_dim, false, [&](auto dh, auto) {
    hipLaunchKernelGGL(attn_fwd_keymask_kernel<dh()>, dim3(8 * a.n8), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
  });
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}
