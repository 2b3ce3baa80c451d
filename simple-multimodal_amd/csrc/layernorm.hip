// LayerNorm forward / backward for the fusion path (nn.LayerNorm at models/fusion_layers.py:205,209).
// HBM-bound: one wavefront owns one row (d <= 2048), 16-byte loads (8 bf16 per lane per chunk),
// f32 statistics by wave butterfly reduction, no LDS in the forward.
// Algorithmic bytes per row: forward 2 x 2d (x in, y out) + 8; backward 3 x 2d (x, dy in; dx out).
#include <type_traits>

#include "mmf_internal.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;     // 4 waves, one row each
constexpr int MAX_CH = 4;              // 4 chunks x 64 lanes x 8 elements = 2048 columns

// Workgroups of a launch (round 3, same box, profiles/r03_layernorm.txt).  Forward, chunk form / lane form: three problems of
// 15,072 rows 13.0 / 9.6 us with 1024 workgroups; all six, 30,144 rows, 20.7 / 16.4 us with 2048.
constexpr int FWD_BLOCKS = 1024, FWD_BLOCKS_LARGE = 2048;
constexpr long long FWD_LARGE_ROWS = 20000;            // more rows than this in one launch: FWD_BLOCKS_LARGE
// Backward: enough rows in flight per CU to cover the HBM latency.  The lane form keeps its next row in flight, so two workgroups
// per CU already do, and fewer partial rows are left for the finalize pass (2048 / 1024 / 512 workgroups 23.5 / 20.5 / 19.9 us per
// three-problem launch, finalize included; the chunk form 25.1 / 24.1 / 23.8).
constexpr int BWD_BLOCKS_LANE = 512;
constexpr int BWD_BLOCKS_CHUNK = 2048;                 // also the bound the workspace is sized for

struct LnArgs {
  int nprob;
  int d;
  float eps;
  float* ws;                             // backward: [total blocks][2][d] partial column sums
  int blk_start[MMF_LN_MAX_PROBLEMS + 1];
  mmf_ln_problem p[MMF_LN_MAX_PROBLEMS];
};

template <int NCH>
__global__ __launch_bounds__(256)
void ln_fwd_kernel(const LnArgs a) {
  const int pi = mmf_group_problem(a.blk_start, a.nprob, blockIdx.x);
  const mmf_ln_problem& P = a.p[pi];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = ((int)blockIdx.x - a.blk_start[pi]) * ROWS_PER_BLOCK + wave;
  if (row >= P.rows) return;
  const int d = a.d;
  const unsigned short* x = static_cast<const unsigned short*>(P.x) + (size_t)row * d;
  float v[NCH][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < d) {
      unpack8(*reinterpret_cast<const u32x4_t*>(x + col), v[c]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[c][e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
    }
  }
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < d) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float t = v[c][e] - mean; q += t * t; }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)d + a.eps);
  unsigned short* y = static_cast<unsigned short*>(P.y) + (size_t)row * d;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < d) {
      const f32x4_t g0 = *reinterpret_cast<const f32x4_t*>(P.gamma + col);
      const f32x4_t g1 = *reinterpret_cast<const f32x4_t*>(P.gamma + col + 4);
      const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(P.beta + col);
      const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(P.beta + col + 4);
      float o[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (v[c][e] - mean) * rstd * g0[e] + b0[e];
        o[e + 4] = (v[c][e + 4] - mean) * rstd * g1[e] + b1[e];
      }
      *reinterpret_cast<u32x4_t*>(y + col) = pack8(o);
    }
  }
  if (lane == 0) { P.mean[row] = mean; P.rstd[row] = rstd; }
}

// Column ownership of the lane form, for d = 512 NV + 256 H8: lane l owns columns [512 c + 8 l, +8) of each of the NV 512-column
// blocks (16-byte bf16 loads) and [512 NV + 4 l, +4) of the last 256 (8-byte loads), so every lane is busy at d = 768 and a lane's
// EP values of a per-column vector (gamma, beta, the dgamma / dbeta sums) stay in registers across rows.  Element 8 c + e of a
// lane is column 512 c + 8 l + e; the last four are columns 512 NV + 4 l + e.
template <int NV, int H8>
struct LaneCols {
  static constexpr int EP = 8 * NV + 4 * H8, D = 512 * NV + 256 * H8;
  struct Bf16 { u32x4_t v[NV > 0 ? NV : 1]; u32x2_t t; };      // a lane's share of one bf16 row, as loaded
  static __device__ __forceinline__ void load(const unsigned short* row, int lane, Bf16& r) {
#pragma unroll
    for (int c = 0; c < NV; ++c) r.v[c] = *reinterpret_cast<const u32x4_t*>(row + 512 * c + 8 * lane);
    if (H8) r.t = *reinterpret_cast<const u32x2_t*>(row + 512 * NV + 4 * lane);
  }
  static __device__ __forceinline__ void unpack(const Bf16& r, float (&f)[EP]) {
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      float t[8];
      unpack8(r.v[c], t);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[8 * c + e] = t[e];
    }
    if (H8) { f[8 * NV] = bf16lo(r.t[0]); f[8 * NV + 1] = bf16hi(r.t[0]); f[8 * NV + 2] = bf16lo(r.t[1]); f[8 * NV + 3] = bf16hi(r.t[1]); }
  }
  static __device__ __forceinline__ void store(unsigned short* row, int lane, const float (&o)[EP]) {
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const u32x4_t w = {pack_bf16x2(o[8 * c], o[8 * c + 1]), pack_bf16x2(o[8 * c + 2], o[8 * c + 3]),
                         pack_bf16x2(o[8 * c + 4], o[8 * c + 5]), pack_bf16x2(o[8 * c + 6], o[8 * c + 7])};
      *reinterpret_cast<u32x4_t*>(row + 512 * c + 8 * lane) = w;
    }
    if (H8) {
      const u32x2_t w = {pack_bf16x2(o[8 * NV], o[8 * NV + 1]), pack_bf16x2(o[8 * NV + 2], o[8 * NV + 3])};
      *reinterpret_cast<u32x2_t*>(row + 512 * NV + 4 * lane) = w;
    }
  }
  static __device__ __forceinline__ void load_f32(const float* p, int lane, float (&f)[EP]) {
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4_t g = *reinterpret_cast<const f32x4_t*>(p + 512 * c + 8 * lane + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[8 * c + 4 * h + e] = g[e];
      }
    if (H8) {
      const f32x4_t g = *reinterpret_cast<const f32x4_t*>(p + 512 * NV + 4 * lane);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[8 * NV + e] = g[e];
    }
  }
  static __device__ __forceinline__ void store_f32(float* p, int lane, const float (&f)[EP]) {
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        *reinterpret_cast<f32x4_t*>(p + 512 * c + 8 * lane + 4 * h) =
            f32x4_t{f[8 * c + 4 * h], f[8 * c + 4 * h + 1], f[8 * c + 4 * h + 2], f[8 * c + 4 * h + 3]};
    if (H8) *reinterpret_cast<f32x4_t*>(p + 512 * NV + 4 * lane) = f32x4_t{f[8 * NV], f[8 * NV + 1], f[8 * NV + 2], f[8 * NV + 3]};
  }
};

// One row of the lane-form forward: a lane's share r of the row -> its normalised, scaled and shifted values o (f32, not yet
// rounded) and the row's statistics.  ln_fwd_lane_kernel and ln2_add3_lane_kernel both normalise through this one routine and must
// agree bit for bit, so which products are fused into the additions behind them is WRITTEN here and not left to the compiler
// (contraction is off in this function): left alone it chose differently in the two kernels — the squares of the variance sum fused
// in one and not in the other — and rstd differed in its last bit.  The choices are the ones the forward kernel was compiled to
// before the routine was shared: squares rounded, then added; variance * (1 / d) + eps and gamma * (x hat) + beta as one fma each.
template <class LC>
__device__ __forceinline__ void ln_lane_row(const typename LC::Bf16& r, const float (&gam)[LC::EP], const float (&bet)[LC::EP],
                                            const float inv_d, const float eps, float (&o)[LC::EP], float& mean, float& rstd) {
#pragma clang fp contract(off)
  constexpr int EP = LC::EP;
  float v[EP];
  LC::unpack(r, v);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < EP; ++e) s += v[e];
  mean = wave_sum(s) * inv_d;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < EP; ++e) {
    v[e] -= mean;
    const float sq = v[e] * v[e];
    q += sq;
  }
  rstd = rsqrtf(__builtin_fmaf(wave_sum(q), inv_d, eps));
#pragma unroll
  for (int e = 0; e < EP; ++e) {
    const float xh = v[e] * rstd;
    o[e] = __builtin_fmaf(gam[e], xh, bet[e]);
  }
}

// Round 3: the forward in the lane form of ln_bwd_lane_kernel below (columns as LaneCols deals them; gamma / beta in registers
// instead of 6 KB of L2 reads per row; a workgroup's waves walk strided rows with the next row's load in flight).
template <int NV, int H8>
__global__ __launch_bounds__(256)
void ln_fwd_lane_kernel(const LnArgs a) {
  using LC = LaneCols<NV, H8>;
  constexpr int EP = LC::EP, d = LC::D;
  const int pi = mmf_group_problem(a.blk_start, a.nprob, blockIdx.x);
  const mmf_ln_problem& P = a.p[pi];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = a.blk_start[pi + 1] - a.blk_start[pi];
  const float inv_d = 1.f / (float)d;
  float gam[EP], bet[EP];
  LC::load_f32(P.gamma, lane, gam);
  LC::load_f32(P.beta, lane, bet);
  auto fetch = [&](int row, typename LC::Bf16& r) { LC::load(static_cast<const unsigned short*>(P.x) + (size_t)row * d, lane, r); };
  const int step = nblk * ROWS_PER_BLOCK;
  int row = ((int)blockIdx.x - a.blk_start[pi]) * ROWS_PER_BLOCK + wave;
  typename LC::Bf16 cur, nxt;
  if (row < P.rows) fetch(row, cur);
  for (; row < P.rows; row += step) {
    const bool more = row + step < P.rows;
    if (more) fetch(row + step, nxt);
    float o[EP], mean, rstd;
    ln_lane_row<LC>(cur, gam, bet, inv_d, a.eps, o, mean, rstd);
    LC::store(static_cast<unsigned short*>(P.y) + (size_t)row * d, lane, o);
    if (lane == 0) { P.mean[row] = mean; P.rstd[row] = rstd; }
    if (more) cur = nxt;
  }
}

// norm2 of two cross-modal blocks and the three-way modality sum behind them in one pass: e = x + LN_a(pre_a) + LN_b(pre_b), the
// rows of pre_a / pre_b normalised by ln_lane_row, each normalised value rounded to bf16 as the tensor ln_fwd_lane_kernel stores
// would hold it, then summed as add3_grouped_kernel sums (x, y_a, y_b): f32, left to right, rounded once.  The two normalised
// tensors (written, then read again by the sum: half the bytes of the two-kernel form) never reach memory; the statistics do, the
// backward works from pre_a / pre_b and them.  Rows are walked as in ln_fwd_lane_kernel, with the next row's three loads in flight.
struct Ln2Add3Args {
  int nprob;
  float eps;
  int blk_start[MMF_LN2_ADD3_MAX_PROBLEMS + 1];
  mmf_ln2_add3_problem p[MMF_LN2_ADD3_MAX_PROBLEMS];
};

template <int NV, int H8>
__global__ __launch_bounds__(256)
void ln2_add3_lane_kernel(const Ln2Add3Args a) {
  using LC = LaneCols<NV, H8>;
  constexpr int EP = LC::EP, d = LC::D;
  const int pi = mmf_group_problem(a.blk_start, a.nprob, blockIdx.x);
  const mmf_ln2_add3_problem& P = a.p[pi];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = a.blk_start[pi + 1] - a.blk_start[pi];
  const float inv_d = 1.f / (float)d;
  float gam_a[EP], bet_a[EP], gam_b[EP], bet_b[EP];
  LC::load_f32(P.gamma_a, lane, gam_a);
  LC::load_f32(P.beta_a, lane, bet_a);
  LC::load_f32(P.gamma_b, lane, gam_b);
  LC::load_f32(P.beta_b, lane, bet_b);
  struct Row { typename LC::Bf16 x, pa, pb; };
  auto fetch = [&](int row, Row& r) {
    LC::load(static_cast<const unsigned short*>(P.pre_a) + (size_t)row * d, lane, r.pa);
    LC::load(static_cast<const unsigned short*>(P.pre_b) + (size_t)row * d, lane, r.pb);
    LC::load(static_cast<const unsigned short*>(P.x) + (size_t)row * d, lane, r.x);
  };
  // the bf16 the forward LayerNorm would have stored, as f32 (pairs as LaneCols::store packs them)
  auto round_bf16 = [](float (&y)[EP]) {
#pragma unroll
    for (int e = 0; e < EP; e += 2) {
      const unsigned w = pack_bf16x2(y[e], y[e + 1]);
      y[e] = bf16lo(w);
      y[e + 1] = bf16hi(w);
    }
  };
  const int step = nblk * ROWS_PER_BLOCK;
  int row = ((int)blockIdx.x - a.blk_start[pi]) * ROWS_PER_BLOCK + wave;
  Row cur, nxt;
  if (row < P.rows) fetch(row, cur);
  for (; row < P.rows; row += step) {
    const bool more = row + step < P.rows;
    if (more) fetch(row + step, nxt);
    float ya[EP], yb[EP], xv[EP], mean_a, rstd_a, mean_b, rstd_b;
    ln_lane_row<LC>(cur.pa, gam_a, bet_a, inv_d, a.eps, ya, mean_a, rstd_a);
    ln_lane_row<LC>(cur.pb, gam_b, bet_b, inv_d, a.eps, yb, mean_b, rstd_b);
    round_bf16(ya);
    round_bf16(yb);
    LC::unpack(cur.x, xv);
#pragma unroll
    for (int e = 0; e < EP; ++e) xv[e] = xv[e] + ya[e] + yb[e];
    LC::store(static_cast<unsigned short*>(P.e) + (size_t)row * d, lane, xv);
    if (lane == 0) { P.mean_a[row] = mean_a; P.rstd_a[row] = rstd_a; P.mean_b[row] = mean_b; P.rstd_b[row] = rstd_b; }
    if (more) cur = nxt;
  }
}

// Backward: a block owns a strided set of rows of ONE problem; each wave walks its rows, keeps the
// dgamma/dbeta partial sums of its columns in registers, the 4 waves combine through LDS and the
// block issues one f32 atomic per column (Guideline 12: reduce on chip, then one atomic per block).
// ADD (mmf_layernorm_bwd_add_grouped): dx = r + that, r = the bf16 rows behind the problem's `y`, added in f32 in front of the one
// rounding; a lane reads its share of r's row right before it stores the same columns of dx, so r may be dx.
template <int NCH, bool ADD>
__global__ __launch_bounds__(256)
void ln_bwd_kernel(const LnArgs a) {
  __shared__ float red[2][3][NCH * 512];          // [dgamma|dbeta][waves 1..3][column]
  const int pi = mmf_group_problem(a.blk_start, a.nprob, blockIdx.x);
  const mmf_ln_problem& P = a.p[pi];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = a.blk_start[pi + 1] - a.blk_start[pi];
  const int d = a.d;
  float dg[NCH][8], db[NCH][8];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) { dg[c][e] = 0.f; db[c][e] = 0.f; }

  for (int row = ((int)blockIdx.x - a.blk_start[pi]) * ROWS_PER_BLOCK + wave; row < P.rows;
       row += nblk * ROWS_PER_BLOCK) {
    const unsigned short* x = static_cast<const unsigned short*>(P.x) + (size_t)row * d;
    const unsigned short* dy = static_cast<const unsigned short*>(P.dy) + (size_t)row * d;
    const float mean = P.mean[row], rstd = P.rstd[row];
    float xh[NCH][8], g[NCH][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = (c * 64 + lane) * 8;
      if (col < d) {
        float xv[8], dv[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(x + col), xv);
        unpack8(*reinterpret_cast<const u32x4_t*>(dy + col), dv);
        const f32x4_t g0 = *reinterpret_cast<const f32x4_t*>(P.gamma + col);
        const f32x4_t g1 = *reinterpret_cast<const f32x4_t*>(P.gamma + col + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float gam = e < 4 ? g0[e] : g1[e - 4];
          xh[c][e] = (xv[e] - mean) * rstd;
          g[c][e] = dv[e] * gam;
          s1 += g[c][e];
          s2 += g[c][e] * xh[c][e];
          dg[c][e] += dv[e] * xh[c][e];
          db[c][e] += dv[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { xh[c][e] = 0.f; g[c][e] = 0.f; }
      }
    }
    const float c1 = wave_sum(s1) / (float)d, c2 = wave_sum(s2) / (float)d;
    unsigned short* dx = static_cast<unsigned short*>(P.dx) + (size_t)row * d;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = (c * 64 + lane) * 8;
      if (col < d) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rstd * (g[c][e] - c1 - xh[c][e] * c2);
        if constexpr (ADD) {
          float rv[8];
          unpack8(*reinterpret_cast<const u32x4_t*>(static_cast<const unsigned short*>(P.y) + (size_t)row * d + col), rv);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] += rv[e];
        }
        *reinterpret_cast<u32x4_t*>(dx + col) = pack8(o);
      }
    }
  }
  // combine the 4 waves' column sums, then one atomic per column per block
  if (wave > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[0][wave - 1][(c * 64 + lane) * 8 + e] = dg[c][e];
        red[1][wave - 1][(c * 64 + lane) * 8 + e] = db[c][e];
      }
  }
  __syncthreads();
  if (wave == 0) {                                 // this workgroup's partials -> workspace row
    float* wsg = a.ws + (size_t)blockIdx.x * 2 * d;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = (c * 64 + lane) * 8;
      if (col < d) {
        f32x4_t g0, g1, b0, b1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float sg = dg[c][e], sb = db[c][e];
#pragma unroll
          for (int w = 0; w < 3; ++w) { sg += red[0][w][col + e]; sb += red[1][w][col + e]; }
          if (e < 4) { g0[e] = sg; b0[e] = sb; } else { g1[e - 4] = sg; b1[e - 4] = sb; }
        }
        *reinterpret_cast<f32x4_t*>(wsg + col) = g0;
        *reinterpret_cast<f32x4_t*>(wsg + col + 4) = g1;
        *reinterpret_cast<f32x4_t*>(wsg + d + col) = b0;
        *reinterpret_cast<f32x4_t*>(wsg + d + col + 4) = b1;
      }
    }
  }
}

// Round 3: the same backward for d = 512 NV + 256 H8 (768 = 512 + 256, 512, 1024, 256 ...) with every lane busy and the
// next row in flight.  ln_bwd_kernel above gives lane l the 16-byte chunks l, l + 64, ...: at d = 768 the second chunk only
// exists for lanes 0-31 (a quarter of the loads and of the arithmetic runs half empty), gamma is re-read from L2 for every
// row (as many bytes as x and dy together), and a wave asks for a row only after it has reduced and stored the one before
// (profiles/r03_layernorm.txt: 2.8 TB/s of algorithmic bytes for the three-problem launches, finalize included).  Here lane l
// owns the columns LaneCols deals it, gamma stays in registers, and the loads of the wave's next row are issued before the
// reductions of the current.  ADD: as in ln_bwd_kernel; r's row travels with x's and dy's, a wave reads a row of r before it
// stores that row of dx and no other wave touches the row, so r may be dx.
template <int NV, int H8, bool ADD>
__global__ __launch_bounds__(256)
void ln_bwd_lane_kernel(const LnArgs a) {
  using LC = LaneCols<NV, H8>;
  constexpr int EP = LC::EP, d = LC::D;               // elements per lane
  __shared__ float red[2][3][64 * EP];                // [dgamma|dbeta][waves 1..3][lane-major element]
  const int pi = mmf_group_problem(a.blk_start, a.nprob, blockIdx.x);
  const mmf_ln_problem& P = a.p[pi];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = a.blk_start[pi + 1] - a.blk_start[pi];
  const float inv_d = 1.f / (float)d;
  float gam[EP], dg[EP], db[EP];
  LC::load_f32(P.gamma, lane, gam);
#pragma unroll
  for (int e = 0; e < EP; ++e) { dg[e] = 0.f; db[e] = 0.f; }

  struct NoRow {};
  struct Row { typename LC::Bf16 x, dy; std::conditional_t<ADD, typename LC::Bf16, NoRow> r; float mean, rstd; };
  auto fetch = [&](int row, Row& r) {
    LC::load(static_cast<const unsigned short*>(P.x) + (size_t)row * d, lane, r.x);
    LC::load(static_cast<const unsigned short*>(P.dy) + (size_t)row * d, lane, r.dy);
    if constexpr (ADD) LC::load(static_cast<const unsigned short*>(P.y) + (size_t)row * d, lane, r.r);
    r.mean = P.mean[row];
    r.rstd = P.rstd[row];
  };
  const int step = nblk * ROWS_PER_BLOCK;
  int row = ((int)blockIdx.x - a.blk_start[pi]) * ROWS_PER_BLOCK + wave;
  Row cur, nxt;
  if (row < P.rows) fetch(row, cur);
  for (; row < P.rows; row += step) {
    const bool more = row + step < P.rows;
    if (more) fetch(row + step, nxt);                  // in flight under this row's reductions and store
    float xv[EP], dv[EP];
    LC::unpack(cur.x, xv);
    LC::unpack(cur.dy, dv);
    const float mean = cur.mean, rstd = cur.rstd;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < EP; ++e) {
      xv[e] = (xv[e] - mean) * rstd;                   // x hat
      const float g = dv[e] * gam[e];
      s1 += g;
      s2 += g * xv[e];
      dg[e] += dv[e] * xv[e];
      db[e] += dv[e];
      dv[e] = g;
    }
    const float c1 = wave_sum(s1) * inv_d, c2 = wave_sum(s2) * inv_d;
    float o[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) o[e] = rstd * (dv[e] - c1 - xv[e] * c2);
    if constexpr (ADD) {
      float rv[EP];
      LC::unpack(cur.r, rv);
#pragma unroll
      for (int e = 0; e < EP; ++e) o[e] += rv[e];
    }
    LC::store(static_cast<unsigned short*>(P.dx) + (size_t)row * d, lane, o);
    if (more) cur = nxt;
  }
  // combine the 4 waves' column sums; this workgroup's partials -> its workspace row (column order)
  if (wave > 0) {
#pragma unroll
    for (int e = 0; e < EP; ++e) { red[0][wave - 1][e * 64 + lane] = dg[e]; red[1][wave - 1][e * 64 + lane] = db[e]; }
  }
  __syncthreads();
  if (wave == 0) {
    float* wsg = a.ws + (size_t)blockIdx.x * 2 * d;
#pragma unroll
    for (int e = 0; e < EP; ++e)
#pragma unroll
      for (int w = 0; w < 3; ++w) { dg[e] += red[0][w][e * 64 + lane]; db[e] += red[1][w][e * 64 + lane]; }
    LC::store_f32(wsg, lane, dg);
    LC::store_f32(wsg + d, lane, db);
  }
}

// second phase: dgamma[j] += sum over the problem's workgroups of their partials.  thread = column,
// blockIdx.z = one of FIN_SLICES slices of the workgroup range; each slice ends in one f32 atomic per
// column (FIN_SLICES adders per address).
constexpr int FIN_SLICES = 64;
__global__ __launch_bounds__(256)
void ln_bwd_finalize_kernel(const LnArgs a) {
  const int pi = blockIdx.y;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= a.d) return;
  const int b0 = a.blk_start[pi], nb = a.blk_start[pi + 1] - b0;
  const int per = (nb + FIN_SLICES - 1) / FIN_SLICES;
  const int lo = b0 + blockIdx.z * per, hi = min(b0 + nb, lo + per);
  if (lo >= hi) return;
  // four independent row loads in flight per thread: written as one running sum the loop is a chain of exposed HBM round
  // trips (16 us per launch for 12 MB of partials, measured in round 2)
  float sg[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
  int b = lo;
  for (; b + 4 <= hi; b += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* w = a.ws + (size_t)(b + u) * 2 * a.d;
      sg[u] += w[col];
      sb[u] += w[a.d + col];
    }
  }
  for (; b < hi; ++b) {
    const float* w = a.ws + (size_t)b * 2 * a.d;
    sg[0] += w[col];
    sb[0] += w[a.d + col];
  }
  atomicAdd(a.p[pi].dgamma + col, (sg[0] + sg[1]) + (sg[2] + sg[3]));
  atomicAdd(a.p[pi].dbeta + col, (sb[0] + sb[1]) + (sb[2] + sb[3]));
}

// the form and instantiation the calling thread's last forward / backward launch took (mmf_layernorm_last_form)
thread_local int t_last_form = 0;

using LnKernel = void (*)(const LnArgs);
// chunk form, by nch = ceil(d / 512); its form id is nch
const LnKernel CHUNK_FWD[MAX_CH] = {ln_fwd_kernel<1>, ln_fwd_kernel<2>, ln_fwd_kernel<3>, ln_fwd_kernel<4>};
const LnKernel CHUNK_BWD[MAX_CH] = {ln_bwd_kernel<1, false>, ln_bwd_kernel<2, false>, ln_bwd_kernel<3, false>, ln_bwd_kernel<4, false>};
const LnKernel CHUNK_BWD_ADD[MAX_CH] = {ln_bwd_kernel<1, true>, ln_bwd_kernel<2, true>, ln_bwd_kernel<3, true>, ln_bwd_kernel<4, true>};
// lane form: the widths d = 512 NV + 256 H8 it is instantiated for
using Ln2Add3Kernel = void (*)(const Ln2Add3Args);
struct LaneWidth { int d, form; LnKernel fwd, bwd, bwd_add; Ln2Add3Kernel fwd2_add3; };   // form id: 100 + 10 NV + H8
template <int NV, int H8>
constexpr LaneWidth lane_width_of() {
  return {LaneCols<NV, H8>::D, 100 + 10 * NV + H8, ln_fwd_lane_kernel<NV, H8>, ln_bwd_lane_kernel<NV, H8, false>,
          ln_bwd_lane_kernel<NV, H8, true>, ln2_add3_lane_kernel<NV, H8>};
}
const LaneWidth LANE_WIDTHS[] = {lane_width_of<0, 1>(), lane_width_of<1, 0>(), lane_width_of<1, 1>(), lane_width_of<2, 0>()};
const LaneWidth* lane_width(int d) {                   // null: d is no lane width
  for (const LaneWidth& w : LANE_WIDTHS) if (w.d == d) return &w;
  return nullptr;
}

int check_common(const char* who, const mmf_ln_problem* p, int n, int d) {
  if (!p || n <= 0 || n > MMF_LN_MAX_PROBLEMS) MMF_FAIL(MMF_E_SHAPE, "%s: num_problems=%d out of range", who, n);
  if (d <= 0 || (d & 7) || d > MAX_CH * 512) MMF_FAIL(MMF_E_SHAPE, "%s: d=%d must be a multiple of 8, <= 2048", who, d);
  return MMF_OK;
}

int full_blocks(int rows) { return (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK; }

// The forward's choice of form for a launch of total_rows rows in `total` one-per-ROWS_PER_BLOCK workgroups: the lane form where
// that would be more workgroups than the budget (a bounded number of them then walk strided rows); else (any other width, or a
// small launch) the chunk form.  The two forms reduce a row in different orders, so what must match the forward bit for bit
// (mmf_layernorm2_add3_available) asks here as well.
int fwd_budget(long long total_rows) { return total_rows > FWD_LARGE_ROWS ? FWD_BLOCKS_LARGE : FWD_BLOCKS; }
bool fwd_takes_lane_form(const LaneWidth* lw, int total, long long total_rows) { return lw && total > fwd_budget(total_rows); }

// A budget of workgroups shared out over the problems in proportion to their rows: at least one each, at most one per
// ROWS_PER_BLOCK rows (so at most budget + num_problems in all).  Fills a.blk_start and returns the total.
template <class Args, class Problem>
int share_blocks(Args& a, const Problem* problems, int num_problems, int budget) {
  long long total_rows = 0;
  for (int i = 0; i < num_problems; ++i) total_rows += problems[i].rows;
  int total = 0;
  for (int i = 0; i < num_problems; ++i) {
    const int rows = problems[i].rows, full = full_blocks(rows);
    const int nb = (int)(((long long)rows * budget + total_rows - 1) / total_rows);
    a.blk_start[i] = total;
    total += nb > full ? full : (nb < 1 ? 1 : nb);
  }
  a.blk_start[num_problems] = total;
  return total;
}

}  // namespace

extern "C" int mmf_layernorm_last_form(void) { return t_last_form; }

extern "C" int mmf_layernorm_fwd_grouped(const mmf_ln_problem* problems, int num_problems, int d,
                                         float eps, void* stream) {
  if (int rc = check_common("mmf_layernorm_fwd_grouped", problems, num_problems, d)) return rc;
  LnArgs a; a.nprob = num_problems; a.d = d; a.eps = eps; a.ws = nullptr;
  int total = 0;                                       // one workgroup per ROWS_PER_BLOCK rows
  long long total_rows = 0;
  for (int i = 0; i < num_problems; ++i) {
    const mmf_ln_problem& p = problems[i];
    if (p.rows <= 0 || !p.x || !p.y || !p.gamma || !p.beta || !p.mean || !p.rstd)
      MMF_FAIL(MMF_E_SHAPE, "mmf_layernorm_fwd_grouped[%d]: null operand or rows=%d", i, p.rows);
    if (!mmf_aligned16(p.x) || !mmf_aligned16(p.y) || !mmf_aligned16(p.gamma) || !mmf_aligned16(p.beta))
      MMF_FAIL(MMF_E_ALIGN, "mmf_layernorm_fwd_grouped[%d]: pointers must be 16-byte aligned", i);
    a.blk_start[i] = total;
    total += full_blocks(p.rows);
    total_rows += p.rows;
    a.p[i] = p;
  }
  a.blk_start[num_problems] = total;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LaneWidth* lw = lane_width(d);
  if (fwd_takes_lane_form(lw, total, total_rows)) {
    total = share_blocks(a, problems, num_problems, fwd_budget(total_rows));
    hipLaunchKernelGGL(lw->fwd, dim3(total), dim3(256), 0, s, a);
    t_last_form = lw->form;
    MMF_CHECK_LAUNCH("mmf_layernorm_fwd_grouped(lane)");
    return MMF_OK;
  }
  const int nch = (d + 511) / 512;
  hipLaunchKernelGGL(CHUNK_FWD[nch - 1], dim3(total), dim3(256), 0, s, a);
  t_last_form = nch;
  MMF_CHECK_LAUNCH("mmf_layernorm_fwd_grouped");
  return MMF_OK;
}

extern "C" int mmf_layernorm2_add3_available(const int32_t* rows, int num_problems, int d) {
  if (!rows || num_problems <= 0 || num_problems > MMF_LN2_ADD3_MAX_PROBLEMS) return 0;
  int total = 0;                                        // the forward launch over pre_a and pre_b of every sum
  long long total_rows = 0;
  for (int i = 0; i < num_problems; ++i) {
    if (rows[i] <= 0) return 0;
    total += 2 * full_blocks(rows[i]);
    total_rows += 2LL * rows[i];
  }
  return fwd_takes_lane_form(lane_width(d), total, total_rows);
}

extern "C" int mmf_layernorm2_add3_fwd_grouped(const mmf_ln2_add3_problem* problems, int num_problems, int d, float eps, void* stream) {
  const char* who = "mmf_layernorm2_add3_fwd_grouped";
  if (!problems || num_problems <= 0 || num_problems > MMF_LN2_ADD3_MAX_PROBLEMS)
    MMF_FAIL(MMF_E_SHAPE, "%s: num_problems=%d out of range", who, num_problems);
  const LaneWidth* lw = lane_width(d);
  if (!lw) MMF_FAIL(MMF_E_SHAPE, "%s: d=%d is no lane width: compose the two launches", who, d);
  Ln2Add3Args a; a.nprob = num_problems; a.eps = eps;
  for (int i = 0; i < num_problems; ++i) {
    const mmf_ln2_add3_problem& p = problems[i];
    if (p.rows <= 0 || !p.x || !p.pre_a || !p.pre_b || !p.e || !p.gamma_a || !p.beta_a || !p.gamma_b || !p.beta_b || !p.mean_a ||
        !p.rstd_a || !p.mean_b || !p.rstd_b)
      MMF_FAIL(MMF_E_SHAPE, "%s[%d]: null operand or rows=%d", who, i, p.rows);
    if (!mmf_aligned16(p.x) || !mmf_aligned16(p.pre_a) || !mmf_aligned16(p.pre_b) || !mmf_aligned16(p.e) || !mmf_aligned16(p.gamma_a) ||
        !mmf_aligned16(p.beta_a) || !mmf_aligned16(p.gamma_b) || !mmf_aligned16(p.beta_b))
      MMF_FAIL(MMF_E_ALIGN, "%s[%d]: pointers must be 16-byte aligned", who, i);
    a.p[i] = p;
  }
  // a row of this launch is three rows read: the workgroup budget of a plain forward of as many rows keeps as many bytes in flight
  const int total = share_blocks(a, problems, num_problems, FWD_BLOCKS);
  hipLaunchKernelGGL(lw->fwd2_add3, dim3(total), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}

extern "C" size_t mmf_layernorm_bwd_workspace_bytes(int d) {
  return (size_t)(BWD_BLOCKS_CHUNK + MMF_LN_MAX_PROBLEMS) * 2 * (size_t)(d > 0 ? d : 0) * sizeof(float);
}

// the two backward entries: `add` = the residual r behind every problem's `y` is added into dx
static int ln_bwd_run(const char* who, const mmf_ln_problem* problems, int num_problems, int d, void* workspace, size_t workspace_bytes,
                      void* stream, bool add) {
  if (int rc = check_common(who, problems, num_problems, d)) return rc;
  if (!workspace || workspace_bytes < mmf_layernorm_bwd_workspace_bytes(d) || !mmf_aligned16(workspace))
    MMF_FAIL(MMF_E_SHAPE, "%s: workspace of %zu bytes (16-byte aligned) required", who, mmf_layernorm_bwd_workspace_bytes(d));
  LnArgs a; a.nprob = num_problems; a.d = d; a.eps = 0.f; a.ws = static_cast<float*>(workspace);
  for (int i = 0; i < num_problems; ++i) {
    const mmf_ln_problem& p = problems[i];
    if (p.rows <= 0 || !p.x || !p.dy || !p.dx || !p.gamma || !p.mean || !p.rstd || !p.dgamma || !p.dbeta || (add && !p.y))
      MMF_FAIL(MMF_E_SHAPE, "%s[%d]: null operand or rows=%d", who, i, p.rows);
    if (!mmf_aligned16(p.x) || !mmf_aligned16(p.dy) || !mmf_aligned16(p.dx) || !mmf_aligned16(p.gamma) || (add && !mmf_aligned16(p.y)))
      MMF_FAIL(MMF_E_ALIGN, "%s[%d]: pointers must be 16-byte aligned", who, i);
    a.p[i] = p;
  }
  // Each workgroup leaves one row of column partials in the workspace (same-row float atomics would run ~14x below the
  // streaming rate: MI355X_MICROARCH.md, Global float atomics), summed by the finalize pass.
  const LaneWidth* lw = lane_width(d);
  const int total = share_blocks(a, problems, num_problems, lw ? BWD_BLOCKS_LANE : BWD_BLOCKS_CHUNK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nch = (d + 511) / 512;
  const LnKernel kernel = lw ? (add ? lw->bwd_add : lw->bwd) : (add ? CHUNK_BWD_ADD : CHUNK_BWD)[nch - 1];
  hipLaunchKernelGGL(kernel, dim3(total), dim3(256), 0, s, a);
  t_last_form = lw ? lw->form : nch;
  MMF_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(ln_bwd_finalize_kernel, dim3((d + 255) / 256, num_problems, FIN_SLICES), dim3(256), 0, s, a);
  MMF_CHECK_LAUNCH(who);
  return MMF_OK;
}

extern "C" int mmf_layernorm_bwd_grouped(const mmf_ln_problem* problems, int num_problems, int d,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return ln_bwd_run("mmf_layernorm_bwd_grouped", problems, num_problems, d, workspace, workspace_bytes, stream, false);
}

extern "C" int mmf_layernorm_bwd_add_grouped(const mmf_ln_problem* problems, int num_problems, int d,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  return ln_bwd_run("mmf_layernorm_bwd_add_grouped", problems, num_problems, d, workspace, workspace_bytes, stream, true);
}
