// The pieces a DeBERTa-v3 forward has and the fusion path did not (mmfusion/deberta.py).
//   embed   word_embeddings[ids] (or f32 inputs_embeds rows) -> LayerNorm in f32 -> * mask -> bf16 rows, one pass
//   attn    fused disentangled attention forward, head_dim 64:
//             s[i][j] = (Q_i.K_j + Q_i.posK[idx(i-j)] + K_j.posQ[idx(i-j)]) / scale, masked softmax over j, @ V
//           Scores, bias and probabilities live in registers and LDS only.  With LSE it also writes the rows' log-sum-exp.
//   backward with respect to the inputs (the weights are frozen; prompt tuning): the embedding LayerNorm's input gradient, and
//           the attention backward: a delta pre-pass, a dQ pass and a dK/dV pass from one kernel body, without atomics.
//   the same backward with the gradient of the position tables posQ | posK (fine-tuning the layer's q / k weights, which also
//           project the relative embeddings): a template flag of the two passes and a fixed-order reduction kernel.
//   full fine-tuning: the embedding backward with the LayerNorm parameters' gradients on either route (per-workgroup partial
//           column sums added in a fixed order), and the scatter-add of gradient rows into the word-embedding table's gradient
//           (the first occurrence of a table row owns it): no atomics in either.
//   training-mode dropout (HuggingFace's model in train()): a DROP template flag of the attention forward and of both backward passes
//           (the probabilities are dropped in front of the product with V; the mask is drawn again, never stored): db_drop_key /
//           db_drop_w, ahead of the forward kernel.  The hidden sites' streaming kernel is mmf_hidden_dropout (elementwise.hip).
// What the forward and the backward must agree on is stated once, as file-local __device__ functions that take operands and
// never the name of their caller: the score tile (db_idx / db_fill_idx, db_chunks, db_pos_rows, db_frag, db_score; ahead of the
// forward kernel) and the embedding LayerNorm's row statistics (db_row_stats).  The backward's P is the forward's P because both
// call db_score on a tile staged by the same functions; the masking and softmax around it are each kernel's.  Bounds that are
// constants of the file stay literals or template arguments inside the helpers: a clamp whose bounds arrive as function arguments
// compiled to other device code in all six attention kernels.
// Left unshared: the four "u32x4 of bf16 -> transposed LDS tile" loops (sVt; sOt with sO2t interleaved; sT).  One function for
// them changed the device code of every attention kernel, whatever its signature, and the dK/dV pass's two tiles cannot interleave
// through it; those four loops are the text they were, and the kernels compile to the instructions they had.
#include <float.h>
#include "mmf_internal.h"

namespace {

constexpr int DB_THREADS = 256;

// mask element `i` of a (n, T) mask given as f32 (kind 1) or u8 (kind 2); kind 0: all ones
__device__ __forceinline__ float db_mask(const void* __restrict__ mask, int kind, size_t i) {
  if (kind == 1) return static_cast<const float*>(mask)[i];
  if (kind == 2) return static_cast<const unsigned char*>(mask)[i] ? 1.0f : 0.0f;
  return 1.0f;
}

__device__ __forceinline__ int db_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// the table row an id names: an id outside the table names its nearest row (the forward's gather, and what its gradient follows)
__device__ __forceinline__ long long db_table_row(long long id, int vocab) { return id < 0 ? 0 : (id >= vocab ? vocab - 1 : id); }

// ---- embeddings ---------------------------------------------------------------------------------------------
// One wave per row; lane l owns columns 4 l + 256 k (k < 4, so d <= 1024), kept in registers between the two statistics
// passes (mean, then the centred second moment: what torch's LayerNorm computes) and the store.
struct DbRowStats { float mean, rstd; };

// the lane's columns of row `src` -> v (zeros past d), and the row's statistics: the forward's and, again, the backward's
__device__ __forceinline__ DbRowStats db_row_stats(const float* __restrict__ src, int lane, int d, float eps, f32x4_t (&v)[4]) {
  float sum = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * lane + 256 * k;
    v[k] = c < d ? *reinterpret_cast<const f32x4_t*>(src + c) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    sum += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  }
  const float mean = wave_sum(sum) / (float)d;
  float sq = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (4 * lane + 256 * k < d) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float c = v[k][e] - mean; sq = fmaf(c, c, sq); }
    }
  }
  return {mean, rsqrtf(wave_sum(sq) / (float)d + eps)};
}

__global__ __launch_bounds__(DB_THREADS)
void deberta_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ embeds, const float* __restrict__ table,
                          const float* __restrict__ gamma, const float* __restrict__ beta, const void* __restrict__ mask,
                          int mask_kind, unsigned short* __restrict__ out, int rows, int d, int vocab, float eps) {
  const int row = blockIdx.x * (DB_THREADS / MMF_WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* __restrict__ src;
  if (ids) {
    src = table + (size_t)db_table_row(ids[row], vocab) * d;       // an id outside the table reads its nearest row, never past it
  } else {
    src = embeds + (size_t)row * d;
  }
  f32x4_t v[4];
  const DbRowStats st = db_row_stats(src, lane, d, eps, v);
  const float mean = st.mean, rstd = st.rstd;
  const float m = db_mask(mask, mask_kind, (size_t)row);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < d) {
      const f32x4_t g = *reinterpret_cast<const f32x4_t*>(gamma + c), b = *reinterpret_cast<const f32x4_t*>(beta + c);
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = (fmaf((v[k][e] - mean) * rstd, g[e], b[e])) * m;
      *reinterpret_cast<u32x2_t*>(out + (size_t)row * d + c) = u32x2_t{pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3])};
    }
  }
}

// ---- disentangled attention ------------------------------------------------------------------------------------
// One workgroup = (64 queries, head, item): 4 waves of 16 queries each, walking the keys in tiles of 32.
// v_mfma_f32_16x16x32_bf16 throughout: lane (q = lane >> 4, r = lane & 15) holds A[row r][k 8q..8q+7], B[k 8q..8q+7][col r]
// and D[row 4q + e][col r].  Every product is formed TRANSPOSED, with the wave's 16 queries as the columns:
//   S^T   [key][query]     A = K tile rows (LDS)           B = Q fragment (registers, loaded once)
//   C2P^T [pos row][query] A = posK rows (global, L2)      B = Q fragment
//   P2C^T [pos row][key]   A = posQ rows (global, L2)      B = K tile rows (LDS)  -- the same LDS fragment as S^T's A
//   O^T   [dh][query]      A = V^T tile rows (LDS)         B = P^T = the softmax of S^T's own D registers, packed to bf16
// so a lane ends with the scores of ONE query (its column) and the row statistics need two shuffles, and the
// probabilities are a B operand without leaving their registers.  S^T's D holds, per 32-key tile, keys 4q..4q+3 of chunk 0
// and 16 + 4q..16 + 4q+3 of chunk 1; the MFMA's k index is only a summation index, so V^T is stored with its keys permuted
// to that order (db_slot) and both operands are one 16-byte read.
//
// The relative-position terms.  idx is non-decreasing in delta = i - j with steps of at most 1 (the caller's contract:
// mmfusion/deberta.py checks the table it builds), so a tile touches a short run of consecutive posK / posQ rows:
//   a wave's 16 queries x 32 keys: 47 deltas -> at most 47 rows from lo_c = idx(smallest delta): 3 row chunks of 16 (C2P)
//   the block's 64 queries x 32 keys: 95 deltas -> at most 95 rows from lo_p: 6 row chunks (P2C, shared by the 4 waves,
//   each forming a quarter of its (row chunk, key chunk) tiles)
// Only the chunks up to idx(largest delta) are formed: far from the diagonal the log buckets make that one or two.  Both
// products are parked in LDS as f32 and each lane gathers its 8 (query, key) entries at idx(delta) - lo.  Every gather
// offset and every row index is clamped, so a table that breaks the contract gives wrong numbers, not a stray access.
//
// LDS: K tile 32 x 72 bf16 (4608 B), V^T 64 x 40 bf16 (5120 B), C2P 4 waves x 16 x 49 f32 (12544 B), P2C 32 x 97 f32
// (12416 B), the tile's 95 idx values and 32 key-mask values: 35.1 KB, four workgroups per CU by LDS.
constexpr int DB_BQ = 64, DB_BK = 32, DB_DH = 64;
constexpr int DB_KLD = 72, DB_VLD = 40, DB_CLD = 49, DB_PLD = 97;
constexpr int DB_CROWS = 48, DB_PROWS = 96, DB_NIDX = DB_BQ + DB_BK - 1;      // 95

__device__ __forceinline__ int db_slot(int key) {            // key of a 32-key tile -> its k slot in the PV product
  const int c = key >> 4, k = key & 15;
  return 8 * (k >> 2) + 4 * c + (k & 3);
}

// The score tile: the pieces the forward and both passes of the backward form s with.  "own" = the 64 tokens of the workgroup
// (a lane's column; the forward's queries), "other" = the 32 tokens of the tile (the forward's keys).

// idx(delta): the delta clamped to the table's +-(T - 1), the value to the rows 0 .. S2 - 1 of posQ | posK.  The only read of
// idx in this file.
__device__ __forceinline__ int db_idx(const int* __restrict__ idx, int delta, int T, int S2) {
  return db_clamp(idx[db_clamp(delta, -(T - 1), T - 1) + T - 1], 0, S2 - 1);
}

// sIdx[t] = idx(d0 + step t) for the tile's 95 deltas; slot t belongs to the pairs with own - other + 31 = t
__device__ __forceinline__ void db_fill_idx(int* __restrict__ sIdx, const int* __restrict__ idx, int tid, int d0, int step, int T, int S2) {
  if (tid < DB_NIDX) sIdx[tid] = db_idx(idx, d0 + step * tid, T, S2);
}

// how many 16-row chunks from row lo reach row hi of a window (the idx values of its two end slots), within the ROWS its LDS
// buffer holds
template <int ROWS>
__device__ __forceinline__ int db_chunks(int lo, int hi) {
  const int n = (hi - lo) / 16 + 1;
  return n < 1 ? 1 : (n > ROWS / 16 ? ROWS / 16 : n);
}

// 16 table rows (this lane: `row` >= 0, clamped to the table's last; tab points at its head's columns 8 q ..) x the two-fragment
// B operand -> the lane's four f32 at dst
__device__ __forceinline__ void db_pos_rows(const unsigned short* __restrict__ tab, int ld_pos, int row, int S2, bf16x8_t b0, bf16x8_t b1,
                                            float* __restrict__ dst) {
  const unsigned short* __restrict__ a = tab + (size_t)(row < S2 - 1 ? row : S2 - 1) * ld_pos;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(a), b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(a + 32), b1, acc, 0, 0, 0);
#pragma unroll
  for (int e = 0; e < 4; ++e) dst[e] = acc[e];
}

// one MFMA fragment of the staged other rows: row `row`, columns 32 ks + 8 q ..
__device__ __forceinline__ bf16x8_t db_frag(const unsigned short* rows, int row, int ks, int q) {
  return *reinterpret_cast<const bf16x8_t*>(rows + row * DB_KLD + ks * 32 + q * 8);
}

// the score of (own token ow of the block = column r of its wave, other token `key` of the tile) from S^T's entry s and the
// two parked position products, gathered at idx(delta) - lo of each window; the offsets clamped to the buffers
__device__ __forceinline__ float db_score(float s, const int* __restrict__ sIdx, const float* __restrict__ cw, const float* __restrict__ sP,
                                          int ow, int r, int key, int lo_c, int lo_p, float inv_scale) {
  const int ix = sIdx[ow - key + (DB_BK - 1)];
  int oc = ix - lo_c, op = ix - lo_p;
  oc = oc < 0 ? 0 : (oc > DB_CROWS - 1 ? DB_CROWS - 1 : oc);
  op = op < 0 ? 0 : (op > DB_PROWS - 1 ? DB_PROWS - 1 : op);
  return (s + cw[r * DB_CLD + oc] + sP[key * DB_PLD + op]) * inv_scale;
}

// Training-mode dropout of the probabilities (HuggingFace: softmax -> dropout -> @ V).  The mask is a function of the element and
// never of the launch: sub-stream (item0 + item) H + h of (state, site), element i T + j for query i and key j (below 2^20), so a
// chunk that starts at item0 draws what the whole batch would, and the backward's two passes, whichever token is "own", draw the
// forward's bit again.  thresh != 0 in every DROP instantiation (the entry points take the plain kernels otherwise).  The arguments
// are one MmfItemDrop (mmf_internal.h), filled and checked by mmf_item_drop_fill.

// A DROP kernel takes one MmfItemDrop behind its other arguments and a plain one takes nothing there (an empty pack), so the plain
// instantiations keep the argument block, and with it the device code, they had before there was a DROP form
__device__ __forceinline__ MmfItemDrop db_drop_of() { return MmfItemDrop{nullptr, 0u, 0u, 0u, 1.0f}; }
__device__ __forceinline__ MmfItemDrop db_drop_of(const MmfItemDrop& dr) { return dr; }

__device__ __forceinline__ unsigned db_drop_key(const MmfItemDrop& dr, int item, int H, int h) {
  return mmf_rng_key(*dr.state, dr.site, (dr.item0 + (unsigned)item) * (unsigned)H + (unsigned)h);
}

// the factor of pair (query i, key j): c where it is kept, 0 where it is dropped
__device__ __forceinline__ float db_drop_w(const MmfItemDrop& dr, unsigned key, int i, int j, int T) {
  return mmf_keep(key, (unsigned)i * (unsigned)T + (unsigned)j, dr.thresh) ? dr.inv_keep : 0.0f;
}

// LSE: also write lse[item][h][i] = m + log(l), what the backward reads.  DROP: the online softmax's m and l, and the lse, run over
// the undropped probabilities; only the bf16 operand of the P V product is keep ? p c : 0
template <bool LSE, bool DROP, typename... Drop>
__global__ __launch_bounds__(DB_THREADS)
void deberta_attn_fwd_kernel(const unsigned short* __restrict__ qkv, const unsigned short* __restrict__ posq,
                             const unsigned short* __restrict__ posk, int ld_pos, const int* __restrict__ idx,
                             const void* __restrict__ mask, int mask_kind, unsigned short* __restrict__ out,
                             float* __restrict__ lse, int H, int T, int S2 /* 2 S */, float inv_scale, const Drop... drop) {
  static_assert(sizeof...(Drop) == (DROP ? 1 : 0), "a DROP kernel takes one MmfItemDrop, a plain one none");
  const MmfItemDrop dr = db_drop_of(drop...);
  __shared__ __attribute__((aligned(16))) unsigned short sK[DB_BK * DB_KLD];
  __shared__ __attribute__((aligned(16))) unsigned short sVt[DB_DH * DB_VLD];
  __shared__ float sC[4 * 16 * DB_CLD];
  __shared__ float sP[DB_BK * DB_PLD];
  __shared__ int sIdx[DB_NIDX + 1];
  __shared__ float sKm[DB_BK];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, r = lane & 15;
  const int i0 = blockIdx.x * DB_BQ, h = blockIdx.y, item = blockIdx.z;
  const int d = H * DB_DH, ld = 3 * d;
  const unsigned short* __restrict__ base = qkv + (size_t)item * T * ld + h * DB_DH;
  const size_t mrow = (size_t)item * T;

  // this lane's query (column r of every product of this wave) and its Q fragment
  const int iq = i0 + wave * 16 + r, iqc = iq < T ? iq : T - 1;
  bf16x8_t qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(base + (size_t)iqc * ld + ks * 32 + q * 8);
  const bool q_on = db_mask(mask, mask_kind, mrow + iqc) != 0.0f;

  f32x4_t o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.0f;
  unsigned dkey = 0u;
  if constexpr (DROP) dkey = db_drop_key(dr, item, H, h);
  float* __restrict__ cw = sC + wave * 16 * DB_CLD;
  const unsigned short* __restrict__ pq = posq + h * DB_DH + q * 8;
  const unsigned short* __restrict__ pk = posk + h * DB_DH + q * 8;

  for (int j0 = 0; j0 < T; j0 += DB_BK) {
    __syncthreads();                                             // the previous tile's readers are done
    {
      // K rows as they are; V transposed with its keys in db_slot order.  Keys past T read row T - 1: they get probability 0.
      const int key = tid >> 3, c8 = (tid & 7) * 8;
      const int j = j0 + key < T ? j0 + key : T - 1;
      const unsigned short* __restrict__ src = base + (size_t)j * ld + c8;
      *reinterpret_cast<u32x4_t*>(sK + key * DB_KLD + c8) = *reinterpret_cast<const u32x4_t*>(src + d);
      const u32x4_t vv = *reinterpret_cast<const u32x4_t*>(src + 2 * d);
      const int slot = db_slot(key);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sVt[(c8 + 2 * e) * DB_VLD + slot] = (unsigned short)(vv[e] & 0xffffu);
        sVt[(c8 + 2 * e + 1) * DB_VLD + slot] = (unsigned short)(vv[e] >> 16);
      }
      db_fill_idx(sIdx, idx, tid, i0 - j0 - (DB_BK - 1), 1, T, S2);          // delta = query - key
      if (tid < DB_BK) sKm[tid] = j0 + tid < T ? db_mask(mask, mask_kind, mrow + j0 + tid) : 0.0f;
    }
    __syncthreads();

    const int lo_p = sIdx[0], hi_p = sIdx[DB_NIDX - 1];
    const int lo_c = sIdx[16 * wave], hi_c = sIdx[16 * wave + 46];
    const int npc = db_chunks<DB_PROWS>(lo_p, hi_p), ncc = db_chunks<DB_CROWS>(lo_c, hi_c);

    // the K fragments of this tile: A of S^T and B of P2C^T
    bf16x8_t kf[2][2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[kc][ks] = db_frag(sK, kc * 16 + r, ks, q);

    // P2C^T: this wave's share of the (row chunk, key chunk) tiles -> sP[key][pos row - lo_p]
    for (int t = wave; t < npc * 2; t += 4) {
      const int rc = t >> 1, kc = t & 1;
      db_pos_rows(pq, ld_pos, lo_p + rc * 16 + r, S2, kc ? kf[1][0] : kf[0][0], kc ? kf[1][1] : kf[0][1],
                  sP + (kc * 16 + r) * DB_PLD + rc * 16 + q * 4);
    }
    // C2P^T: this wave's own rows -> cw[query][pos row - lo_c]
    for (int c = 0; c < ncc; ++c) db_pos_rows(pk, ld_pos, lo_c + c * 16 + r, S2, qf[0], qf[1], cw + r * DB_CLD + c * 16 + q * 4);
    // S^T
    f32x4_t s[2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      s[kc] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s[kc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kc][ks], qf[ks], s[kc], 0, 0, 0);
    }
    __syncthreads();                                             // sP (all waves) and cw are complete

    // gather the two bias terms, mask, online softmax; lane (q, r): keys kc * 16 + 4 q + e of query r
    float p[2][4], tmax = -INFINITY;
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = kc * 16 + q * 4 + e;
        float v = db_score(s[kc][e], sIdx, cw, sP, 16 * wave + r, r, key, lo_c, lo_p, inv_scale);
        if (!(q_on && sKm[key] != 0.0f)) v = -FLT_MAX;          // a masked pair: HuggingFace's masked_fill(finfo.min)
        if (j0 + key >= T) v = -INFINITY;                        // no such key
        p[kc][e] = v;
        tmax = fmaxf(tmax, v);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);                      // finite: every tile has at least one key below T
    const float alpha = __expf(m_run - m_new);
    float psum = 0.0f;
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[kc][e] = __expf(p[kc][e] - m_new);                     // a fully masked row: exp(0) = 1 on every key, the uniform row
        psum += p[kc][e];
      }
    l_run = l_run * alpha + psum;                                // this lane's keys only; the four q groups are summed at the end
    m_run = m_new;
    if constexpr (DROP) {                                        // after the row sum: l takes the undropped probabilities
#pragma unroll
      for (int kc = 0; kc < 2; ++kc)
#pragma unroll
        for (int e = 0; e < 4; ++e) p[kc][e] *= db_drop_w(dr, dkey, iq, j0 + kc * 16 + q * 4 + e, T);
    }
    const u32x4_t pw = {pack_bf16x2(p[0][0], p[0][1]), pack_bf16x2(p[0][2], p[0][3]), pack_bf16x2(p[1][0], p[1][1]), pack_bf16x2(p[1][2], p[1][3])};
    const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(sVt + (t * 16 + r) * DB_VLD + q * 8);
      o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[t] * alpha, 0, 0, 0);
    }
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  if (iq < T) {
    const float inv = 1.0f / l_run;
    unsigned short* __restrict__ dst = out + ((size_t)item * T + iq) * d + h * DB_DH + q * 4;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      *reinterpret_cast<u32x2_t*>(dst + t * 16) = u32x2_t{pack_bf16x2(o[t][0] * inv, o[t][1] * inv), pack_bf16x2(o[t][2] * inv, o[t][3] * inv)};
    // a fully masked row: m = -FLT_MAX and l = T, so the sum is -FLT_MAX again in f32; the backward does not use it
    if (LSE && q == 0) lse[((size_t)item * H + h) * T + iq] = m_run + logf(l_run);
  }
}

// ---- backward with respect to the inputs (prompt tuning through the frozen layers) --------------------------------
// embeddings: d_embeds = mask[row] * the LayerNorm input gradient of the bf16 gradient dy of deberta_embed_kernel's output
// (inputs_embeds route).  The row statistics are the forward's (db_row_stats); one wave per row, same lane map.
// What the two embedding-backward kernels agree on, for one row: on entry v holds the lane's columns of the source row (what
// db_row_stats left); on return v holds the normalised values xh, dyv the lane's columns of the bf16 gradient `dyrow`, g =
// dy * gamma * mask (the gradient of the normalised value), and the result the row means s1 = mean g, s2 = mean g xh
struct DbRowMeans { float s1, s2; };
__device__ __forceinline__ DbRowMeans db_row_grad(const unsigned short* __restrict__ dyrow, const float* __restrict__ gamma, float m,
                                                  float mean, float rstd, int lane, int d, f32x4_t (&v)[4], f32x4_t (&dyv)[4],
                                                  f32x4_t (&g)[4]) {
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * lane + 256 * k;
    g[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    dyv[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (c < d) {
      const u32x2_t w = *reinterpret_cast<const u32x2_t*>(dyrow + c);
      const f32x4_t gm = *reinterpret_cast<const f32x4_t*>(gamma + c);
      dyv[k] = f32x4_t{bf16lo(w[0]), bf16hi(w[0]), bf16lo(w[1]), bf16hi(w[1])};
      g[k] = dyv[k] * gm * m;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[k][e] = (v[k][e] - mean) * rstd;
        s1 += g[k][e];
        s2 = fmaf(g[k][e], v[k][e], s2);
      }
    }
  }
  return {wave_sum(s1) / (float)d, wave_sum(s2) / (float)d};
}

// the lane's columns 4 lane + 256 k .. + 3 of the row's input gradient, rstd (g - s1 - xh s2); a masked row: exactly 0.  The fused
// multiply-add is spelled out: left to the compiler's contraction, one kernel fused all four column groups and the other three and
// a half of them, and the two kernels' bits must agree
__device__ __forceinline__ f32x4_t db_row_dx(const f32x4_t& g, const f32x4_t& xh, float m, float rstd, DbRowMeans s) {
  f32x4_t o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = m != 0.0f ? rstd * fmaf(-s.s2, xh[e], g[e] - s.s1) : 0.0f;
  return o;
}

__global__ __launch_bounds__(DB_THREADS)
void deberta_embed_bwd_kernel(const float* __restrict__ embeds, const float* __restrict__ gamma, const void* __restrict__ mask,
                              int mask_kind, const unsigned short* __restrict__ dy, float* __restrict__ dx, int rows, int d, float eps) {
  const int row = blockIdx.x * (DB_THREADS / MMF_WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* __restrict__ src = embeds + (size_t)row * d;
  const float m = db_mask(mask, mask_kind, (size_t)row);
  f32x4_t v[4], dyv[4], g[4];
  const DbRowStats st = db_row_stats(src, lane, d, eps, v);
  const DbRowMeans s = db_row_grad(dy + (size_t)row * d, gamma, m, st.mean, st.rstd, lane, d, v, dyv, g);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < d) *reinterpret_cast<f32x4_t*>(dx + (size_t)row * d + c) = db_row_dx(g[k], v[k], m, st.rstd, s);
  }
}

// The same backward with the parameters' gradients (fine-tuning the embeddings), on either route of deberta_embed_kernel: the source
// row is table[db_table_row(id)] or the row of embeds itself.  A workgroup's 4 waves walk the rows 4 b + wave, + 4 gridDim.x, ...,
// one wave per row with the lane map above; d_rows (written, or added to with `accumulate`) has the bits of deberta_embed_bwd_kernel
// for the same operands, by db_row_grad / db_row_dx.  Each lane keeps dgamma = sum dy mask xh and dbeta = sum dy mask of its
// columns over the wave's rows in registers; the 4 waves combine through LDS in wave order and the workgroup leaves one row
// [dgamma | dbeta] of partials in `part` (gridDim.x, 2 d): no atomics.  A row with mask 0 is not read: zeros (nothing with
// `accumulate`) in d_rows and nothing in the sums.  deberta_embed_params_finalize_kernel adds the partial rows in order.
constexpr int DB_PARAM_BLOCKS = 512;            // at most this many workgroups (= partial rows in the workspace)

__global__ __launch_bounds__(DB_THREADS)
void deberta_embed_bwd_params_kernel(const long long* __restrict__ ids, const float* __restrict__ embeds, const float* __restrict__ table,
                                     const float* __restrict__ gamma, const void* __restrict__ mask, int mask_kind,
                                     const unsigned short* __restrict__ dy, float* __restrict__ dx, int accumulate,
                                     float* __restrict__ part, int rows, int d, int vocab, float eps) {
  __shared__ float red[2][3][1024];             // [dgamma | dbeta][waves 1 .. 3][column]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4_t dg[4], db[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { dg[k] = f32x4_t{0.f, 0.f, 0.f, 0.f}; db[k] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
  const long long step = (long long)gridDim.x * (DB_THREADS / MMF_WAVE);
  for (long long row = (long long)blockIdx.x * (DB_THREADS / MMF_WAVE) + wave; row < rows; row += step) {
    const float m = db_mask(mask, mask_kind, (size_t)row);
    float* __restrict__ dst = dx + (size_t)row * d;
    if (m == 0.0f) {
      if (!accumulate) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = 4 * lane + 256 * k;
          if (c < d) *reinterpret_cast<f32x4_t*>(dst + c) = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
      }
      continue;
    }
    const float* __restrict__ src = ids ? table + (size_t)db_table_row(ids[row], vocab) * d : embeds + (size_t)row * d;
    f32x4_t v[4], dyv[4], g[4];
    const DbRowStats st = db_row_stats(src, lane, d, eps, v);
    const DbRowMeans s = db_row_grad(dy + (size_t)row * d, gamma, m, st.mean, st.rstd, lane, d, v, dyv, g);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * lane + 256 * k;
      if (c < d) {
        f32x4_t o = db_row_dx(g[k], v[k], m, st.rstd, s);
        if (accumulate) o += *reinterpret_cast<const f32x4_t*>(dst + c);
        *reinterpret_cast<f32x4_t*>(dst + c) = o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dm = dyv[k][e] * m;
          dg[k][e] = fmaf(dm, v[k][e], dg[k][e]);
          db[k][e] += dm;
        }
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * lane + 256 * k;
      *reinterpret_cast<f32x4_t*>(&red[0][wave - 1][c]) = dg[k];
      *reinterpret_cast<f32x4_t*>(&red[1][wave - 1][c]) = db[k];
    }
  }
  __syncthreads();
  if (wave == 0) {
    float* __restrict__ out = part + (size_t)blockIdx.x * 2 * d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * lane + 256 * k;
      if (c < d) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          dg[k] += *reinterpret_cast<const f32x4_t*>(&red[0][w][c]);
          db[k] += *reinterpret_cast<const f32x4_t*>(&red[1][w][c]);
        }
        *reinterpret_cast<f32x4_t*>(out + c) = dg[k];
        *reinterpret_cast<f32x4_t*>(out + d + c) = db[k];
      }
    }
  }
}

// dgamma[c] += the sum over the `nblk` partial rows of column c, dbeta[c] += that of column d + c: one lane per column, the rows in
// order through four running sums (independent loads in flight), combined in a fixed order
__global__ __launch_bounds__(DB_THREADS)
void deberta_embed_params_finalize_kernel(const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta, int nblk, int d) {
  const int col = blockIdx.x * DB_THREADS + threadIdx.x;
  if (col >= 2 * d) return;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int b = 0;
  for (; b + 4 <= nblk; b += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] += part[(size_t)(b + u) * 2 * d + col];
  }
  for (; b < nblk; ++b) s[0] += part[(size_t)b * 2 * d + col];
  float* __restrict__ dst = col < d ? dgamma + col : dbeta + (col - d);
  *dst += (s[0] + s[1]) + (s[2] + s[3]);
}

// dtable[db_table_row(ids[r])] += d_rows[r] over the unmasked rows r, without atomics and without a sort: the first unmasked
// occurrence of a table row owns it.  One wave per row p: it scans ids[0 .. p) 64 at a time (coalesced loads, one ballot per step) and
// leaves if an earlier unmasked row names the same table row; otherwise it walks ids[p .. rows) the same way and adds the matching
// unmasked rows to its registers in ascending row order (p itself first), then reads, adds to and writes the table row once.  Every
// table element is written by one lane, once; a table row no unmasked id names is not touched; a masked row is never read.
// The known cost is a very frequent id: one wave sums all its occurrences.
__global__ __launch_bounds__(DB_THREADS)
void embedding_scatter_add_kernel(const long long* __restrict__ ids, const void* __restrict__ mask, int mask_kind,
                                  const float* __restrict__ d_rows, float* __restrict__ dtable, int rows, int d, int vocab) {
  const int p = blockIdx.x * (DB_THREADS / MMF_WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= rows) return;
  if (db_mask(mask, mask_kind, (size_t)p) == 0.0f) return;
  const long long own = db_table_row(ids[p], vocab);
  auto names_own = [&](int q, int end) {
    return q < end && db_mask(mask, mask_kind, (size_t)q) != 0.0f && db_table_row(ids[q], vocab) == own;
  };
  for (int q0 = 0; q0 < p; q0 += MMF_WAVE)
    if (__ballot(names_own(q0 + lane, p))) return;             // (wave-uniform) an earlier row owns this table row
  f32x4_t acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int q0 = p; q0 < rows; q0 += MMF_WAVE) {
    unsigned long long hits = __ballot(names_own(q0 + lane, rows));
    while (hits) {
      const int j = __ffsll((long long)hits) - 1;
      hits &= hits - 1;
      const float* __restrict__ src = d_rows + (size_t)(q0 + j) * d;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = 4 * lane + 256 * k;
        if (c < d) acc[k] += *reinterpret_cast<const f32x4_t*>(src + c);
      }
    }
  }
  float* __restrict__ dst = dtable + (size_t)own * d;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < d) *reinterpret_cast<f32x4_t*>(dst + c) = *reinterpret_cast<const f32x4_t*>(dst + c) + acc[k];
  }
}

// delta[item][h][i] = sum_d dO_i O_i of one head: one lane per (token, head), eight 16-byte reads of each operand
__global__ __launch_bounds__(DB_THREADS)
void deberta_attn_delta_kernel(const unsigned short* __restrict__ out, const unsigned short* __restrict__ dout, float* __restrict__ delta,
                               int H, int T, unsigned total /* n T H */) {
  const unsigned i = blockIdx.x * DB_THREADS + threadIdx.x;
  if (i >= total) return;
  const unsigned row = i / (unsigned)H, h = i - row * (unsigned)H, item = row / (unsigned)T, t = row - item * (unsigned)T;
  const size_t off = ((size_t)row * H + h) * DB_DH;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < DB_DH / 8; ++k) {
    float a[8], b[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(out + off + 8 * k), a);
    unpack8(*reinterpret_cast<const u32x4_t*>(dout + off + 8 * k), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(a[e], b[e], acc);
  }
  delta[((size_t)item * H + h) * T + t] = acc;
}

// The attention backward, both passes from one body.  The score is symmetric under (Q, posK, i) <-> (K, posQ, j):
//   s_ij = Q_i.K_j + Q_i.posK[idx(i-j)] + K_j.posQ[idx(i-j)]
// so with "own" = the 64 tokens a workgroup owns (a lane's column, as the forward's queries) and "other" = the tokens it
// walks in tiles of 32, the dQ pass (KPASS false: own = queries, other = keys) and the dK/dV pass (KPASS true: own = keys,
// other = queries, the delta negated) run the same products with the operands swapped:
//   S^T    [other][own]     A = other rows (LDS)                  B = own fragment: Q | K (registers)
//   T1^T   [pos row][own]   A = posK | posQ rows (global)         B = own fragment          -- the wave's 47-delta window
//   T2^T   [pos row][other] A = posQ | posK rows (global)         B = other rows (LDS)      -- the block's 95-delta window
//   dP^T   [other][own]     A = V | dO rows of the tile (LDS)     B = own dO | V fragment
//   dOwn^T [dh][own]       += A = other^T (LDS, db_slot order)    B = dS^T, the lane's own D registers packed to bf16
//   dOwn^T [dh][own]       += A = posK^T | posQ^T window (LDS)    B = the bucket sums of dS over the window rows
//   dV^T   [dh][own key]   += A = dO^T (LDS, db_slot order)       B = P^T packed to bf16            (KPASS only)
// P = exp(s - lse_i), or 1/T on a masked query row; dS = P (dP - delta_i) / scale on unmasked pairs, else 0.
//
// The position-gradient term.  For one own token the others of a tile that gather the same position row are a contiguous
// run (idx is monotone in delta), so sFirst / sEnd hold, per window row, the run of the tile's 95 deltas that maps to it and
// the lane that holds (own r, rows 8 q .. 8 q + 7 of a 32-row chunk) as its B operand sums that run of its own token's dS
// row, parked in LDS as f32, in key order: no atomics, the same order every run.
//
// LDS: other rows 32 x 72 and their transpose 64 x 40 (9728 B), V | dO rows and (KPASS) dO^T (9728 B), T1 / dS 4 waves x 16 x 49
// f32 (12544 B), T2 32 x 97 f32 (12416 B), the transposed position window 64 x 104 bf16 (13312 B), idx / run / per-row
// values (1.5 KB): 59.3 KB, two workgroups per CU by LDS.
//
// The table gradients (POS; fine-tuning: the layer's q / k weights also project the relative embeddings).  The gradient of the
// table a pass gathers with its own token's vector is "bucket sums x the own token's vector":
//   dposK[r] += sum_i A_ir Q_i (dQ pass)      dposQ[r] += sum_j B_jr K_j (dK/dV pass)
// i.e. the contraction over the block's 64 own tokens of the very bf16 sums the position term's B operand holds.  The sums go
// through LDS (sA, in T2's buffer, which is free once the scores are gathered) to become the A operand, own tokens along k;
// the B operand is the own tokens' vectors transposed, 16 head columns per wave, held in registers from the start:
//   dTab [pos row][dh]      A = bucket sums [pos row][own] (LDS)  B = own^T [own][dh] (registers)
// and the 16 x 16 results go to the workgroup's OWN (2S, 64) f32 partial table in global memory (`part`): no other workgroup
// touches it, and the lanes of this one that meet at an address in successive tiles (the window moves with the tile) are
// ordered by the tile's barriers.  The partial table is never cleared: idx is monotone, so the windows of successive tiles
// overlap and move one way, a row outside the previous tile's window has not been written yet and is STORED, a row inside it
// is added to; what a workgroup leaves behind is the rows idx(its smallest delta) .. idx(its largest delta), every one
// written.  deberta_pos_reduce_kernel works that range out again and sums those rows of the partial tables in a fixed order.
// Own tokens past T contribute zeros (their own^T entries are 0).
constexpr int DB_TLD = 104, DB_TROWS = 96;
constexpr int DB_ALD = 64;                                   // sA: 96 window rows x 64 own tokens bf16, 8-token groups XOR-swizzled by row

//
// DROP (the forward dropped the probabilities, db_drop_w above): with w_ij = keep_ij c, dP_ij = w_ij (dO_i . V_j) and the dV product
// takes w_ij P_ij; dS = P (dP - delta) / scale as without, delta_i = dO_i . O_i still being the row sum of P dP because O is the
// dropped product.  The bucket sums and the table gradients come from this dS with no further change.
template <bool KPASS, bool POS, bool DROP, typename... Drop>
__global__ __launch_bounds__(DB_THREADS)
void deberta_attn_bwd_kernel(const unsigned short* __restrict__ qkv, const unsigned short* __restrict__ posq,
                             const unsigned short* __restrict__ posk, int ld_pos, const int* __restrict__ idx,
                             const void* __restrict__ mask, int mask_kind, const float* __restrict__ lse,
                             const unsigned short* __restrict__ dout, const float* __restrict__ delta,
                             unsigned short* __restrict__ dqkv, float* part /* POS: this pass's partial tables */,
                             int H, int T, int S2 /* 2 S */, float inv_scale, const Drop... drop) {
  static_assert(sizeof...(Drop) == (DROP ? 1 : 0), "a DROP kernel takes one MmfItemDrop, a plain one none");
  const MmfItemDrop dr = db_drop_of(drop...);
  static_assert(DB_TROWS * DB_ALD * 2 <= DB_BK * DB_PLD * 4, "sA must fit T2's buffer");
  __shared__ __attribute__((aligned(16))) unsigned short sO[DB_BK * DB_KLD];          // other rows: K | Q
  __shared__ __attribute__((aligned(16))) unsigned short sOt[DB_DH * DB_VLD];         // their transpose, db_slot order
  __shared__ __attribute__((aligned(16))) unsigned short sO2[DB_BK * DB_KLD];         // V | dO rows of the other tokens
  __shared__ __attribute__((aligned(16))) unsigned short sO2t[KPASS ? DB_DH * DB_VLD : 8];   // dO^T, db_slot order
  __shared__ __attribute__((aligned(16))) unsigned short sT[DB_DH * DB_TLD];          // posK^T | posQ^T over the block's window
  __shared__ float sC[4 * 16 * DB_CLD];
  __shared__ __attribute__((aligned(16))) float sP[DB_BK * DB_PLD];
  __shared__ int sIdx[DB_NIDX + 1], sFirst[DB_TROWS], sEnd[DB_TROWS];
  __shared__ float sOm[DB_BK], sLse[DB_BK], sDl[DB_BK];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, r = lane & 15;
  const int own0 = blockIdx.x * DB_BQ, h = blockIdx.y, item = blockIdx.z;
  const int d = H * DB_DH, ld = 3 * d;
  const unsigned short* __restrict__ base = qkv + (size_t)item * T * ld + h * DB_DH;
  const unsigned short* __restrict__ dob = dout + (size_t)item * T * d + h * DB_DH;
  const size_t mrow = (size_t)item * T, srow = ((size_t)item * H + h) * T;

  // this lane's own token (column r of every product of this wave): its Q | K fragment and its dO | V fragment
  const int ow = wave * 16 + r, io = own0 + ow, ioc = io < T ? io : T - 1;
  const unsigned short* __restrict__ own = base + (size_t)ioc * ld + (KPASS ? d : 0);
  const unsigned short* __restrict__ own2 = KPASS ? base + (size_t)ioc * ld + 2 * d : dob + (size_t)ioc * d;
  bf16x8_t xf[2], yf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    xf[ks] = *reinterpret_cast<const bf16x8_t*>(own + ks * 32 + q * 8);
    yf[ks] = *reinterpret_cast<const bf16x8_t*>(own2 + ks * 32 + q * 8);
  }
  const bool own_on = db_mask(mask, mask_kind, mrow + ioc) != 0.0f;
  const float lse_o = KPASS ? 0.0f : lse[srow + ioc], dl_o = KPASS ? 0.0f : delta[srow + ioc];
  const float inv_T = 1.0f / (float)T;
  unsigned dkey = 0u;
  if constexpr (DROP) dkey = db_drop_key(dr, item, H, h);

  f32x4_t acc[4], accv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = accv[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float* __restrict__ cw = sC + wave * 16 * DB_CLD;
  const unsigned short* __restrict__ tab1 = (KPASS ? posq : posk) + h * DB_DH;        // gathered with the own token's vector
  const unsigned short* __restrict__ tab2 = (KPASS ? posk : posq) + h * DB_DH + q * 8;

  // POS: own^T, B[k = own token ks * 32 + 8 q + e][col = head column 16 wave + r]; the partial table of this workgroup
  bf16x8_t xt[2];
  unsigned short* const sA = reinterpret_cast<unsigned short*>(sP);
  float* const ptab = POS ? part + (((size_t)item * gridDim.x + blockIdx.x) * H + h) * ((size_t)S2 * DB_DH) + wave * 16 + r : nullptr;
  if (POS) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4_t w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t0 = own0 + ks * 32 + q * 8 + 2 * e;
        const unsigned lo = t0 < T ? base[(size_t)t0 * ld + (KPASS ? d : 0) + wave * 16 + r] : 0u;
        const unsigned hi = t0 + 1 < T ? base[(size_t)(t0 + 1) * ld + (KPASS ? d : 0) + wave * 16 + r] : 0u;
        w[e] = lo | (hi << 16);
      }
      xt[ks] = __builtin_bit_cast(bf16x8_t, w);
    }
  }

  int plo = S2, phi = -1;                                        // POS: the previous tile's window (none yet)
  for (int o0 = 0; o0 < T; o0 += DB_BK) {
    __syncthreads();                                             // the previous tile's readers are done
    {
      // other rows as they are and transposed with their tokens in db_slot order.  Tokens past T read row T - 1: P and dS are 0 there.
      const int key = tid >> 3, c8 = (tid & 7) * 8;
      const int j = o0 + key < T ? o0 + key : T - 1;
      const unsigned short* __restrict__ srcA = base + (size_t)j * ld + c8 + (KPASS ? 0 : d);
      const unsigned short* __restrict__ srcB = KPASS ? dob + (size_t)j * d + c8 : base + (size_t)j * ld + c8 + 2 * d;
      const u32x4_t va = *reinterpret_cast<const u32x4_t*>(srcA), vb = *reinterpret_cast<const u32x4_t*>(srcB);
      *reinterpret_cast<u32x4_t*>(sO + key * DB_KLD + c8) = va;
      *reinterpret_cast<u32x4_t*>(sO2 + key * DB_KLD + c8) = vb;
      const int slot = db_slot(key);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sOt[(c8 + 2 * e) * DB_VLD + slot] = (unsigned short)(va[e] & 0xffffu);
        sOt[(c8 + 2 * e + 1) * DB_VLD + slot] = (unsigned short)(va[e] >> 16);
        if (KPASS) {
          sO2t[(c8 + 2 * e) * DB_VLD + slot] = (unsigned short)(vb[e] & 0xffffu);
          sO2t[(c8 + 2 * e + 1) * DB_VLD + slot] = (unsigned short)(vb[e] >> 16);
        }
      }
      // slot tid: the pairs with own - other + 31 = tid; delta = query - key is own - other, or other - own in the dK/dV pass
      const int sgn = KPASS ? -1 : 1;
      db_fill_idx(sIdx, idx, tid, sgn * (own0 - o0 - (DB_BK - 1)), sgn, T, S2);
      if (tid < DB_TROWS) { sFirst[tid] = 0; sEnd[tid] = 0; }    // an empty run
      if (tid < DB_BK) {
        const int jj = o0 + tid < T ? o0 + tid : T - 1;
        sOm[tid] = o0 + tid < T ? db_mask(mask, mask_kind, mrow + jj) : 0.0f;
        if (KPASS) { sLse[tid] = lse[srow + jj]; sDl[tid] = delta[srow + jj]; }
      }
    }
    __syncthreads();

    // idx is monotone over the tile's deltas (non-decreasing, or non-increasing in the dK/dV pass): the windows' ends
    const int e0 = sIdx[0], e1 = sIdx[DB_NIDX - 1], w0 = sIdx[16 * wave], w1 = sIdx[16 * wave + 46];
    const int lo_p = e0 < e1 ? e0 : e1, hi_p = e0 < e1 ? e1 : e0;
    const int lo_c = w0 < w1 ? w0 : w1, hi_c = w0 < w1 ? w1 : w0;
    const int npc = db_chunks<DB_PROWS>(lo_p, hi_p), ncc = db_chunks<DB_CROWS>(lo_c, hi_c);
    const int nb32 = (npc + 1) >> 1;                            // 32-row chunks of the block's window

    if (tid < DB_NIDX) {                                         // the run of deltas that gathers each window row
      const int me = sIdx[tid], row = db_clamp(me - lo_p, 0, DB_TROWS - 1);
      if (tid == 0 || sIdx[tid - 1] != me) sFirst[row] = tid;
      if (tid == DB_NIDX - 1 || sIdx[tid + 1] != me) sEnd[row] = tid + 1;
    }
    for (int i = tid; i < nb32 * 32 * 8; i += DB_THREADS) {     // posK^T | posQ^T over the window, rows clamped to the table
      const int row = i >> 3, c8 = (i & 7) * 8;
      int prow = lo_p + row;
      prow = prow > S2 - 1 ? S2 - 1 : prow;
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(tab1 + (size_t)prow * ld_pos + c8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sT[(c8 + 2 * e) * DB_TLD + row] = (unsigned short)(w[e] & 0xffffu);
        sT[(c8 + 2 * e + 1) * DB_TLD + row] = (unsigned short)(w[e] >> 16);
      }
    }

    // the other rows' fragments: A of S^T and B of T2^T
    bf16x8_t kf[2][2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) kf[kc][ks] = db_frag(sO, kc * 16 + r, ks, q);

    // T2^T: this wave's share of the (row chunk, other chunk) tiles -> sP[other][pos row - lo_p]
    for (int t = wave; t < npc * 2; t += 4) {
      const int rc = t >> 1, kc = t & 1;
      db_pos_rows(tab2, ld_pos, lo_p + rc * 16 + r, S2, kc ? kf[1][0] : kf[0][0], kc ? kf[1][1] : kf[0][1],
                  sP + (kc * 16 + r) * DB_PLD + rc * 16 + q * 4);
    }
    // T1^T: this wave's own rows -> cw[own][pos row - lo_c]
    for (int c = 0; c < ncc; ++c) db_pos_rows(tab1 + q * 8, ld_pos, lo_c + c * 16 + r, S2, xf[0], xf[1], cw + r * DB_CLD + c * 16 + q * 4);
    // S^T and dP^T
    f32x4_t s[2], dp[2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      s[kc] = dp[kc] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        s[kc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kc][ks], xf[ks], s[kc], 0, 0, 0);
        const bf16x8_t o2 = db_frag(sO2, kc * 16 + r, ks, q);
        dp[kc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(o2, yf[ks], dp[kc], 0, 0, 0);
      }
    }
    __syncthreads();                                             // sP, cw, sT and the runs are complete

    // lane (q, r): others kc * 16 + 4 q + e of own token r.  The probabilities and dS of the tile stay in registers.
    float p[2][4], ds[2][4];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = kc * 16 + q * 4 + e;
        const float v = db_score(s[kc][e], sIdx, cw, sP, ow, r, key, lo_c, lo_p, inv_scale);
        const bool there = o0 + key < T;                         // the other token exists
        const bool q_on = KPASS ? sOm[key] != 0.0f : own_on, k_on = KPASS ? own_on : sOm[key] != 0.0f;
        const float l = KPASS ? sLse[key] : lse_o, dl = KPASS ? sDl[key] : dl_o;
        const float pe = q_on ? (k_on ? __expf(v - l) : 0.0f) : inv_T;     // a masked query row is the uniform row; its lse is not used
        if constexpr (DROP) {
          const float w = KPASS ? db_drop_w(dr, dkey, o0 + key, io, T) : db_drop_w(dr, dkey, io, o0 + key, T);
          p[kc][e] = there ? pe * w : 0.0f;
          ds[kc][e] = (there && q_on && k_on) ? pe * (dp[kc][e] * w - dl) * inv_scale : 0.0f;
        } else {
          p[kc][e] = there ? pe : 0.0f;
          ds[kc][e] = (there && q_on && k_on) ? pe * (dp[kc][e] - dl) * inv_scale : 0.0f;
        }
      }
    __syncthreads();                                             // every lane has gathered from cw: it becomes the dS rows
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int e = 0; e < 4; ++e) cw[r * DB_CLD + kc * 16 + q * 4 + e] = ds[kc][e];
    __syncthreads();

    const u32x4_t dw = {pack_bf16x2(ds[0][0], ds[0][1]), pack_bf16x2(ds[0][2], ds[0][3]), pack_bf16x2(ds[1][0], ds[1][1]), pack_bf16x2(ds[1][2], ds[1][3])};
    const bf16x8_t df = __builtin_bit_cast(bf16x8_t, dw);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bf16x8_t of = *reinterpret_cast<const bf16x8_t*>(sOt + (t * 16 + r) * DB_VLD + q * 8);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(of, df, acc[t], 0, 0, 0);
    }
    if (KPASS) {
      const u32x4_t pw = {pack_bf16x2(p[0][0], p[0][1]), pack_bf16x2(p[0][2], p[0][3]), pack_bf16x2(p[1][0], p[1][1]), pack_bf16x2(p[1][2], p[1][3])};
      const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8_t of = *reinterpret_cast<const bf16x8_t*>(sO2t + (t * 16 + r) * DB_VLD + q * 8);
        accv[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(of, pf, accv[t], 0, 0, 0);
      }
    }
    // the bucket sums of this lane's own token over window rows c * 32 + 8 q + e, then (posK^T | posQ^T) . sums
    for (int c = 0; c < nb32; ++c) {
      float a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int row = c * 32 + q * 8 + e;
        int t0 = sFirst[row], t1 = sEnd[row];                    // deltas t0 .. t1 - 1; other = ow + 31 - t must lie in the tile
        t0 = t0 < ow ? ow : t0;
        t1 = t1 > ow + DB_BK ? ow + DB_BK : t1;
        float sum = 0.0f;
        for (int t = t0; t < t1; ++t) sum += cw[r * DB_CLD + (ow + (DB_BK - 1) - t)];
        a[e] = sum;
      }
      const u32x4_t aw = pack8(a);
      const bf16x8_t af = __builtin_bit_cast(bf16x8_t, aw);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bf16x8_t tf = *reinterpret_cast<const bf16x8_t*>(sT + (t * 16 + r) * DB_TLD + c * 32 + q * 8);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf, af, acc[t], 0, 0, 0);
      }
      if (POS) {                                                 // the same bf16 sums -> sA[window row][own token]
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int row = c * 32 + q * 8 + e;
          sA[row * DB_ALD + ((((ow >> 3) ^ (row & 7)) << 3) | (ow & 7))] = (unsigned short)((e & 1) ? aw[e >> 1] >> 16 : aw[e >> 1] & 0xffffu);
        }
      }
    }
    if (POS) {
      __syncthreads();                                           // sA is complete
      for (int rc = 0; rc < npc; ++rc) {
        f32x4_t g = {0.f, 0.f, 0.f, 0.f};
        const int row = rc * 16 + r;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8_t sf = *reinterpret_cast<const bf16x8_t*>(sA + row * DB_ALD + (((ks * 4 + q) ^ (row & 7)) << 3));
          g = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf, xt[ks], g, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int prow = lo_p + rc * 16 + q * 4 + e;          // hi_p <= 2 S - 1: never a row past the table
          if (prow <= hi_p) {
            float* dst = ptab + (size_t)prow * DB_DH;
            *dst = (prow < plo || prow > phi) ? g[e] : *dst + g[e];      // first write of this row | a row of the previous window
          }
        }
      }
      plo = lo_p;
      phi = hi_p;
    }
  }
  if (io < T) {
    unsigned short* __restrict__ dst = dqkv + ((size_t)item * T + io) * ld + (KPASS ? d : 0) + h * DB_DH + q * 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      *reinterpret_cast<u32x2_t*>(dst + t * 16) = u32x2_t{pack_bf16x2(acc[t][0], acc[t][1]), pack_bf16x2(acc[t][2], acc[t][3])};
      if (KPASS) *reinterpret_cast<u32x2_t*>(dst + d + t * 16) = u32x2_t{pack_bf16x2(accv[t][0], accv[t][1]), pack_bf16x2(accv[t][2], accv[t][3])};
    }
  }
}

// dposk | dposq (2S, H 64) f32 += the sum over the workgroups (item, block of 64 own tokens) of the dQ | dK/dV pass of the rows
// their partial tables hold, block by block and item by item: one lane per element.  A workgroup of block b wrote the rows
// idx(its smallest delta) .. idx(its largest delta): db_idx again, the function the pass fills sIdx with, at those two deltas, so
// the deltas and idx values are clamped as the pass clamps them by construction.  The rest of its table is not read.
__global__ __launch_bounds__(DB_THREADS)
void deberta_pos_reduce_kernel(const float* __restrict__ part, const int* __restrict__ idx, float* __restrict__ dposq,
                               float* __restrict__ dposk, int ld_dpos, int H, int T, int S2, int n, int nblk) {
  const unsigned i = blockIdx.x * DB_THREADS + threadIdx.x;
  const unsigned width = (unsigned)H * DB_DH;
  if (i >= (unsigned)S2 * width) return;
  const int row = (int)(i / width);
  const unsigned col = i - (unsigned)row * width, h = col >> 6, dh = col & 63;
  const bool kpass = blockIdx.y != 0;
  const size_t stride = (size_t)H * S2 * DB_DH;
  const float* __restrict__ src = part + (size_t)blockIdx.y * n * nblk * stride + ((size_t)h * S2 + row) * DB_DH + dh;
  const int o_last = ((T - 1) / DB_BK) * DB_BK;
  float sum = 0.0f;
  for (int b = 0; b < nblk; ++b) {
    // slot 0 of the block's last tile and slot 94 of its first: own - other at its smallest and largest, negated as the dK/dV pass does
    const int sgn = kpass ? -1 : 1;
    const int r0 = db_idx(idx, sgn * (b * DB_BQ - o_last - (DB_BK - 1)), T, S2), r1 = db_idx(idx, sgn * (b * DB_BQ + DB_BQ - 1), T, S2);
    if (row < (r0 < r1 ? r0 : r1) || row > (r0 < r1 ? r1 : r0)) continue;
#pragma unroll 4
    for (int item = 0; item < n; ++item) sum += src[((size_t)item * nblk + b) * stride];
  }
  float* __restrict__ dst = (kpass ? dposq : dposk) + (size_t)row * ld_dpos + col;
  *dst += sum;
}

int db_mask_check(const char* fn, const void* mask, int mask_kind) {
  if (mask_kind < 0 || mask_kind > 2 || (mask_kind == 0) != (mask == nullptr))
    MMF_FAIL(MMF_E_SHAPE, "%s: mask_kind=%d (0 none, 1 f32, 2 u8) does not match the mask pointer", fn, mask_kind);
  if (mask_kind == 1 && (reinterpret_cast<uintptr_t>(mask) & 3u)) MMF_FAIL(MMF_E_ALIGN, "%s: an f32 mask must be 4-byte aligned", fn);
  return MMF_OK;
}

// what the two embedding entries share: the limits of the one-wave-per-row kernels, the mask, and their grid
int db_embed_rows(const char* fn, int64_t rows, int d, const void* mask, int mask_kind, dim3* grid) {
  if ((d & 3) || d > 1024 || rows > ((int64_t)1 << 31) - 4)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: d=%d (multiple of 4, at most 1024), rows=%lld (below 2^31)", fn, d, (long long)rows);
  if (int rc = db_mask_check(fn, mask, mask_kind)) return rc;
  const int per = DB_THREADS / MMF_WAVE;
  *grid = dim3((unsigned)((rows + per - 1) / per));
  return MMF_OK;
}

}  // namespace

extern "C" int mmf_deberta_embed(const int64_t* ids, const float* embeds, const float* table, const float* gamma, const float* beta,
                                 float eps, const void* mask, int mask_kind, void* out_bf16, int64_t rows, int d, int vocab,
                                 void* stream) {
  if ((ids == nullptr) == (embeds == nullptr)) MMF_FAIL(MMF_E_SHAPE, "mmf_deberta_embed: exactly one of ids / embeds");
  if (!gamma || !beta || !out_bf16 || (ids && !table) || rows <= 0 || d <= 0 || (ids && vocab <= 0))
    MMF_FAIL(MMF_E_SHAPE, "mmf_deberta_embed: null operand or rows=%lld d=%d vocab=%d", (long long)rows, d, vocab);
  dim3 grid;
  if (int rc = db_embed_rows("mmf_deberta_embed", rows, d, mask, mask_kind, &grid)) return rc;
  if (!mmf_aligned16(gamma) || !mmf_aligned16(beta) || !mmf_aligned16(out_bf16) || (ids && !mmf_aligned16(table)) || (embeds && !mmf_aligned16(embeds))
      || (reinterpret_cast<uintptr_t>(ids) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "mmf_deberta_embed: table / embeds / gamma / beta / out must be 16-byte aligned, ids 8-byte aligned");
  hipLaunchKernelGGL(deberta_embed_kernel, grid, dim3(DB_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(ids), embeds, table, gamma, beta, mask, mask_kind, static_cast<unsigned short*>(out_bf16),
                     (int)rows, d, vocab, eps);
  MMF_CHECK_LAUNCH("mmf_deberta_embed");
  return MMF_OK;
}

namespace {

// the checks the attention entries share; `out` is the forward's output (the backward reads it)
int db_attn_check(const char* fn, const void* qkv, const void* posq, const void* posk, int ld_pos, const int* idx, const void* mask,
                  int mask_kind, const void* out, int n, int H, int T, int S, int head_dim, float scale) {
  if (!qkv || !posq || !posk || !idx || !out || n <= 0 || H <= 0 || T <= 0 || S <= 0 || head_dim <= 0 || !(scale > 0.0f))
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or n=%d H=%d T=%d S=%d head_dim=%d scale=%g", fn, n, H, T, S, head_dim, (double)scale);
  if (head_dim == DB_DH && ld_pos < H * DB_DH) MMF_FAIL(MMF_E_SHAPE, "%s: ld_pos=%d is less than H * 64 = %d", fn, ld_pos, H * DB_DH);
  if (head_dim != DB_DH || T > 1024 || S > 256 || n > 65535 || H > 65535)
    MMF_FAIL(MMF_E_UNSUPPORTED, "%s: head_dim=%d (64 only), T=%d (at most 1024), S=%d (at most 256), n=%d H=%d (at most 65535)",
             fn, head_dim, T, S, n, H);
  if (int rc = db_mask_check(fn, mask, mask_kind)) return rc;
  if (!mmf_aligned16(qkv) || !mmf_aligned16(posq) || !mmf_aligned16(posk) || !mmf_aligned16(out) || (ld_pos & 7)
      || (reinterpret_cast<uintptr_t>(idx) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "%s: qkv / posq / posk / out must be 16-byte aligned, ld_pos a multiple of 8, idx 4-byte aligned", fn);
  return MMF_OK;
}

template <bool LSE, bool DROP, typename... Drop>
void db_attn_fwd_launch(const void* qkv, const void* posq, const void* posk, int ld_pos, const int* idx, const void* mask, int mask_kind,
                        void* out, float* lse, int n, int H, int T, int S, float scale, void* stream, const Drop... drop) {
  hipLaunchKernelGGL((deberta_attn_fwd_kernel<LSE, DROP, Drop...>), dim3((T + DB_BQ - 1) / DB_BQ, H, n), dim3(DB_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned short*>(qkv), static_cast<const unsigned short*>(posq),
                     static_cast<const unsigned short*>(posk), ld_pos, idx, mask, mask_kind, static_cast<unsigned short*>(out), lse,
                     H, T, 2 * S, 1.0f / scale, drop...);
}

}  // namespace

extern "C" int mmf_deberta_attn_fwd(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                    const void* mask, int mask_kind, void* out_bf16, int n, int H, int T, int S, int head_dim,
                                    float scale, void* stream) {
  if (int rc = db_attn_check("mmf_deberta_attn_fwd", qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, n, H, T, S, head_dim, scale))
    return rc;
  db_attn_fwd_launch<false, false>(qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, nullptr, n, H, T, S, scale, stream);
  MMF_CHECK_LAUNCH("mmf_deberta_attn_fwd");
  return MMF_OK;
}

extern "C" int mmf_deberta_attn_fwd_lse(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                        const void* mask, int mask_kind, void* out_bf16, float* lse, int n, int H, int T, int S,
                                        int head_dim, float scale, void* stream) {
  const char* fn = "mmf_deberta_attn_fwd_lse";
  if (!lse) MMF_FAIL(MMF_E_SHAPE, "%s: null lse", fn);
  if (int rc = db_attn_check(fn, qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, n, H, T, S, head_dim, scale)) return rc;
  if (reinterpret_cast<uintptr_t>(lse) & 3u) MMF_FAIL(MMF_E_ALIGN, "%s: lse must be 4-byte aligned", fn);
  db_attn_fwd_launch<true, false>(qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, n, H, T, S, scale, stream);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_deberta_attn_fwd_drop(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                         const void* mask, int mask_kind, void* out_bf16, float* lse, int n, int H, int T, int S,
                                         int head_dim, float scale, float p, const uint64_t* rng_state, uint32_t site, int64_t item0,
                                         void* stream) {
  const char* fn = "mmf_deberta_attn_fwd_drop";
  MmfItemDrop dr;
  if (int rc = mmf_item_drop_fill(fn, p, rng_state, site, item0, &dr)) return rc;
  if (int rc = db_attn_check(fn, qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, n, H, T, S, head_dim, scale)) return rc;
  if (reinterpret_cast<uintptr_t>(lse) & 3u) MMF_FAIL(MMF_E_ALIGN, "%s: lse must be 4-byte aligned", fn);
#define DB_FWD(LSE, DROP, ...) db_attn_fwd_launch<LSE, DROP>(qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, n, H, T, S, \
                                                         scale, stream, ##__VA_ARGS__)
  if (dr.thresh == 0u) { if (lse) DB_FWD(true, false); else DB_FWD(false, false); }
  else                 { if (lse) DB_FWD(true, true, dr); else DB_FWD(false, true, dr); }
#undef DB_FWD
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

namespace {

size_t db_pos_workspace_bytes(int n, int H, int T, int S) {      // two passes x (item, block of 64 tokens, head) x (2S, 64) f32
  return (size_t)2 * n * ((T + DB_BQ - 1) / DB_BQ) * H * (2 * (size_t)S) * DB_DH * sizeof(float);
}

// both attention-backward entries: the checks they share, then delta, the dQ pass and the dK/dV pass; POS: the table gradients too
template <bool POS, bool DROP, typename... Drop>
int db_attn_bwd(const char* fn, const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16, float* delta_ws,
                void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale, float* dposq, float* dposk, int ld_dpos,
                void* workspace, size_t workspace_bytes, void* stream, const Drop... drop) {
  if (!lse || !dout_bf16 || !delta_ws || !dqkv_bf16) MMF_FAIL(MMF_E_SHAPE, "%s: null lse / dout / delta_ws / dqkv", fn);
  if (POS && (!dposq || !dposk || !workspace)) MMF_FAIL(MMF_E_SHAPE, "%s: null dposq / dposk / workspace", fn);
  if (int rc = db_attn_check(fn, qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, n, H, T, S, head_dim, scale)) return rc;
  if (POS && ld_dpos < H * DB_DH) MMF_FAIL(MMF_E_SHAPE, "%s: ld_dpos=%d is less than H * 64 = %d", fn, ld_dpos, H * DB_DH);
  if (POS && workspace_bytes < db_pos_workspace_bytes(n, H, T, S))
    MMF_FAIL(MMF_E_SHAPE, "%s: workspace of %zu bytes, %zu needed (mmf_deberta_attn_bwd_pos_workspace_bytes)", fn, workspace_bytes,
             db_pos_workspace_bytes(n, H, T, S));
  if (!mmf_aligned16(dout_bf16) || !mmf_aligned16(dqkv_bf16) || ((reinterpret_cast<uintptr_t>(lse) | reinterpret_cast<uintptr_t>(delta_ws)) & 3u))
    MMF_FAIL(MMF_E_ALIGN, "%s: dout / dqkv must be 16-byte aligned, lse / delta_ws 4-byte aligned", fn);
  if (POS && (!mmf_aligned16(dposq) || !mmf_aligned16(dposk) || !mmf_aligned16(workspace) || (ld_dpos & 3)))
    MMF_FAIL(MMF_E_ALIGN, "%s: dposq / dposk / workspace must be 16-byte aligned, ld_dpos a multiple of 4", fn);
  if ((int64_t)n * T * H >= (int64_t)1 << 31) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: n * T * H = %lld (below 2^31)", fn, (long long)n * T * H);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned short *qkv = static_cast<const unsigned short*>(qkv_bf16), *pq = static_cast<const unsigned short*>(posq_bf16),
                       *pk = static_cast<const unsigned short*>(posk_bf16), *dout = static_cast<const unsigned short*>(dout_bf16);
  unsigned short* dqkv = static_cast<unsigned short*>(dqkv_bf16);
  const unsigned total = (unsigned)((int64_t)n * T * H);
  const dim3 grid((T + DB_BQ - 1) / DB_BQ, H, n);
  float* part = static_cast<float*>(workspace);
  const size_t pass_elems = POS ? db_pos_workspace_bytes(n, H, T, S) / (2 * sizeof(float)) : 0;
  hipLaunchKernelGGL(deberta_attn_delta_kernel, dim3((total + DB_THREADS - 1) / DB_THREADS), dim3(DB_THREADS), 0, s,
                     static_cast<const unsigned short*>(out_bf16), dout, delta_ws, H, T, total);
  MMF_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL((deberta_attn_bwd_kernel<false, POS, DROP, Drop...>), grid, dim3(DB_THREADS), 0, s, qkv, pq, pk, ld_pos, idx, mask, mask_kind, lse, dout,
                     static_cast<const float*>(delta_ws), dqkv, part, H, T, 2 * S, 1.0f / scale, drop...);
  MMF_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL((deberta_attn_bwd_kernel<true, POS, DROP, Drop...>), grid, dim3(DB_THREADS), 0, s, qkv, pq, pk, ld_pos, idx, mask, mask_kind, lse, dout,
                     static_cast<const float*>(delta_ws), dqkv, POS ? part + pass_elems : part, H, T, 2 * S, 1.0f / scale, drop...);
  MMF_CHECK_LAUNCH(fn);
  if (POS) {
    const unsigned elems = (unsigned)(2 * S) * H * DB_DH;
    hipLaunchKernelGGL(deberta_pos_reduce_kernel, dim3((elems + DB_THREADS - 1) / DB_THREADS, 2), dim3(DB_THREADS), 0, s, part, idx, dposq, dposk,
                       ld_dpos, H, T, 2 * S, n, (int)grid.x);
    MMF_CHECK_LAUNCH(fn);
  }
  return MMF_OK;
}

}  // namespace

extern "C" int mmf_deberta_attn_bwd(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                    const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                                    float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale, void* stream) {
  return db_attn_bwd<false, false>("mmf_deberta_attn_bwd", qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, dout_bf16,
                            delta_ws, dqkv_bf16, n, H, T, S, head_dim, scale, nullptr, nullptr, 0, nullptr, 0, stream);
}

extern "C" size_t mmf_deberta_attn_bwd_pos_workspace_bytes(int n, int H, int T, int S) {
  return n > 0 && H > 0 && T > 0 && S > 0 ? db_pos_workspace_bytes(n, H, T, S) : 0;
}

extern "C" int mmf_deberta_attn_bwd_pos(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                        const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                                        float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale,
                                        float* dposq, float* dposk, int ld_dpos, void* workspace, size_t workspace_bytes, void* stream) {
  return db_attn_bwd<true, false>("mmf_deberta_attn_bwd_pos", qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, dout_bf16,
                           delta_ws, dqkv_bf16, n, H, T, S, head_dim, scale, dposq, dposk, ld_dpos, workspace, workspace_bytes, stream);
}

extern "C" int mmf_deberta_attn_bwd_drop(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                         const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                                         float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale,
                                         float p, const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream) {
  const char* fn = "mmf_deberta_attn_bwd_drop";
  MmfItemDrop dr;
  if (int rc = mmf_item_drop_fill(fn, p, rng_state, site, item0, &dr)) return rc;
  if (dr.thresh == 0u)
    return db_attn_bwd<false, false>(fn, qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, dout_bf16, delta_ws, dqkv_bf16,
                                     n, H, T, S, head_dim, scale, nullptr, nullptr, 0, nullptr, 0, stream);
  return db_attn_bwd<false, true>(fn, qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, dout_bf16, delta_ws, dqkv_bf16,
                                  n, H, T, S, head_dim, scale, nullptr, nullptr, 0, nullptr, 0, stream, dr);
}

extern "C" int mmf_deberta_attn_bwd_pos_drop(const void* qkv_bf16, const void* posq_bf16, const void* posk_bf16, int ld_pos, const int* idx,
                                             const void* mask, int mask_kind, const void* out_bf16, const float* lse, const void* dout_bf16,
                                             float* delta_ws, void* dqkv_bf16, int n, int H, int T, int S, int head_dim, float scale,
                                             float* dposq, float* dposk, int ld_dpos, void* workspace, size_t workspace_bytes, float p,
                                             const uint64_t* rng_state, uint32_t site, int64_t item0, void* stream) {
  const char* fn = "mmf_deberta_attn_bwd_pos_drop";
  MmfItemDrop dr;
  if (int rc = mmf_item_drop_fill(fn, p, rng_state, site, item0, &dr)) return rc;
  if (dr.thresh == 0u)
    return db_attn_bwd<true, false>(fn, qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, dout_bf16, delta_ws, dqkv_bf16,
                                    n, H, T, S, head_dim, scale, dposq, dposk, ld_dpos, workspace, workspace_bytes, stream);
  return db_attn_bwd<true, true>(fn, qkv_bf16, posq_bf16, posk_bf16, ld_pos, idx, mask, mask_kind, out_bf16, lse, dout_bf16, delta_ws, dqkv_bf16,
                                 n, H, T, S, head_dim, scale, dposq, dposk, ld_dpos, workspace, workspace_bytes, stream, dr);
}

extern "C" int mmf_deberta_embed_bwd(const float* embeds, const float* gamma, float eps, const void* mask, int mask_kind,
                                     const void* dout_bf16, float* d_embeds, int64_t rows, int d, void* stream) {
  const char* fn = "mmf_deberta_embed_bwd";
  if (!embeds || !gamma || !dout_bf16 || !d_embeds || rows <= 0 || d <= 0) MMF_FAIL(MMF_E_SHAPE, "%s: null operand or rows=%lld d=%d", fn, (long long)rows, d);
  dim3 grid;
  if (int rc = db_embed_rows(fn, rows, d, mask, mask_kind, &grid)) return rc;
  if (!mmf_aligned16(embeds) || !mmf_aligned16(gamma) || !mmf_aligned16(d_embeds) || (reinterpret_cast<uintptr_t>(dout_bf16) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "%s: embeds / gamma / d_embeds must be 16-byte aligned, dout 8-byte aligned", fn);
  hipLaunchKernelGGL(deberta_embed_bwd_kernel, grid, dim3(DB_THREADS), 0, static_cast<hipStream_t>(stream),
                     embeds, gamma, mask, mask_kind, static_cast<const unsigned short*>(dout_bf16), d_embeds, (int)rows, d, eps);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

namespace {

int db_param_blocks(int64_t rows) {
  const int64_t per = DB_THREADS / MMF_WAVE, blocks = (rows + per - 1) / per;
  return (int)(blocks < DB_PARAM_BLOCKS ? blocks : DB_PARAM_BLOCKS);
}

}  // namespace

extern "C" size_t mmf_deberta_embed_bwd_params_workspace_bytes(int64_t rows, int d) {
  return rows > 0 && d > 0 ? (size_t)db_param_blocks(rows) * 2 * (size_t)d * sizeof(float) : 0;
}

extern "C" int mmf_deberta_embed_bwd_params(const int64_t* ids, const float* embeds, const float* table, int vocab, const float* gamma,
                                            float eps, const void* mask, int mask_kind, const void* dout_bf16, float* d_rows,
                                            int accumulate, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                            int64_t rows, int d, void* stream) {
  const char* fn = "mmf_deberta_embed_bwd_params";
  if ((ids == nullptr) == (embeds == nullptr)) MMF_FAIL(MMF_E_SHAPE, "%s: exactly one of ids / embeds", fn);
  if (!gamma || !dout_bf16 || !d_rows || !dgamma || !dbeta || !workspace || (ids && !table) || rows <= 0 || d <= 0 || (ids && vocab <= 0))
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or rows=%lld d=%d vocab=%d", fn, (long long)rows, d, vocab);
  dim3 grid;
  if (int rc = db_embed_rows(fn, rows, d, mask, mask_kind, &grid)) return rc;
  const size_t need = mmf_deberta_embed_bwd_params_workspace_bytes(rows, d);
  if (workspace_bytes < need)
    MMF_FAIL(MMF_E_SHAPE, "%s: workspace of %zu bytes, %zu needed (mmf_deberta_embed_bwd_params_workspace_bytes)", fn, workspace_bytes, need);
  if (!mmf_aligned16(gamma) || !mmf_aligned16(d_rows) || !mmf_aligned16(dgamma) || !mmf_aligned16(dbeta) || !mmf_aligned16(workspace)
      || (ids && !mmf_aligned16(table)) || (embeds && !mmf_aligned16(embeds)) || (reinterpret_cast<uintptr_t>(dout_bf16) & 7u)
      || (reinterpret_cast<uintptr_t>(ids) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "%s: table / embeds / gamma / d_rows / dgamma / dbeta / workspace must be 16-byte aligned, dout and ids 8-byte aligned", fn);
  const int nblk = db_param_blocks(rows);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(deberta_embed_bwd_params_kernel, dim3(nblk), dim3(DB_THREADS), 0, s, reinterpret_cast<const long long*>(ids), embeds, table,
                     gamma, mask, mask_kind, static_cast<const unsigned short*>(dout_bf16), d_rows, accumulate ? 1 : 0, part, (int)rows, d,
                     vocab, eps);
  MMF_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(deberta_embed_params_finalize_kernel, dim3((2 * d + DB_THREADS - 1) / DB_THREADS), dim3(DB_THREADS), 0, s,
                     static_cast<const float*>(part), dgamma, dbeta, nblk, d);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}

extern "C" int mmf_embedding_scatter_add_f32(const int64_t* ids, const void* mask, int mask_kind, const float* d_rows, float* dtable,
                                             int64_t rows, int d, int vocab, void* stream) {
  const char* fn = "mmf_embedding_scatter_add_f32";
  if (!ids || !d_rows || !dtable || rows <= 0 || d <= 0 || vocab <= 0)
    MMF_FAIL(MMF_E_SHAPE, "%s: null operand or rows=%lld d=%d vocab=%d", fn, (long long)rows, d, vocab);
  if (rows > ((int64_t)1 << 30)) MMF_FAIL(MMF_E_UNSUPPORTED, "%s: rows=%lld (at most 2^30)", fn, (long long)rows);
  dim3 grid;
  if (int rc = db_embed_rows(fn, rows, d, mask, mask_kind, &grid)) return rc;
  if (!mmf_aligned16(d_rows) || !mmf_aligned16(dtable) || (reinterpret_cast<uintptr_t>(ids) & 7u))
    MMF_FAIL(MMF_E_ALIGN, "%s: d_rows / dtable must be 16-byte aligned, ids 8-byte aligned", fn);
  hipLaunchKernelGGL(embedding_scatter_add_kernel, grid, dim3(DB_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(ids), mask, mask_kind, d_rows, dtable, (int)rows, d, vocab);
  MMF_CHECK_LAUNCH(fn);
  return MMF_OK;
}
