// Adaptive score normalisation (AS-norm, snorm.py): cohort statistics of unit rows and the normalised top-k over profiles.
//
//   score_tile            the scoring core of both entry points: a 64 x 128 tile of A B^T (unit fp32 rows, d columns) on the fp32-input MFMA
//                         (v_mfma_f32_32x32x2_f32: exact fp32, bitwise an fmaf chain).  A and B pass through LDS in chunks of 32 columns; four
//                         waves, each 32 rows x 64 columns = two 32 x 32 accumulators.  Every score is ONE chain over the d columns in ONE
//                         order (inside a group of 8 columns: 0, 4, 1, 5, 2, 6, 3, 7 - lane half h feeds column 4 h + s at step s), rows and
//                         columns outside the matrices are zeros: a score does not depend on its tile position, on N or on M's tail.
//   snorm_scores_kernel   epilogue 1: the tile goes to the score block S [rows][M] of the workspace.
//   snorm_select_kernel   one workgroup per row of S: radix select (4 x 8 bits, LDS histograms with INTEGER atomics) on the order-preserving
//                         uint32 key of the fp32 score finds the K-th largest value t and the count c of scores strictly above it; then
//                         mean = (sum_{s > t} s + (K - c) t) / K and var = (sum_{s > t} (s - mean)^2 + (K - c) (t - mean)^2) / K in float64:
//                         a thread adds its columns (tid, tid + 256, ..) in ascending order, the 256 partial sums meet in a fixed tree (block_sum, reduce.hpp).
//   snorm_topk_kernel     epilogue 2: z = ((s - mean_e) / std_e + (s - mean_p) / std_p) / 2 in float64, a running top-4 per (row, 32-column
//                         part) across the profile tiles, merged at the end; ties to the lower profile, a NaN z never wins.
//
// No floating-point atomics; one owner per output element; every sum in a fixed order: two runs agree bit for bit.
#include "common.hpp"

namespace {

constexpr int SN_NT = 256;
constexpr int SN_BM = 64, SN_BN = 128;      // tile of the workgroup: rows of A x rows of B
constexpr int SN_KC = 32;                   // columns staged per step
constexpr int SN_LD = SN_KC + 4;            // LDS row stride in floats: 16-byte reads of 16 consecutive rows fall on 64 different banks
constexpr int SN_MAX_D = 512;
constexpr int SN_MAX_M = 1 << 20;
constexpr int SN_MAX_TOPK = 4;
constexpr size_t SN_BLOCK_BYTES = (size_t)64 << 20;   // score block of a row block: at most this (stays cache-resident), ..
constexpr int SN_MIN_BLOCK_ROWS = 64;                 // .. at least one tile of rows ..
constexpr int SN_MAX_BLOCK_ROWS = 1024;               // .. and at most 1024 rows
constexpr float SN_STD_FLOOR = 1e-6f;

// rows of a row block for a cohort of M rows
inline int sn_block_rows(int M) {
  int64_t r = (int64_t)(SN_BLOCK_BYTES / ((size_t)M * sizeof(float)));
  r -= r % SN_BM;
  if (r < SN_MIN_BLOCK_ROWS) r = SN_MIN_BLOCK_ROWS;
  if (r > SN_MAX_BLOCK_ROWS) r = SN_MAX_BLOCK_ROWS;
  return (int)r;
}
inline int sn_alloc_rows(int N, int M) {
  const int rb = sn_block_rows(M);
  return N < 1 ? 1 : (N < rb ? N : rb);
}

typedef float SnTileRow[SN_LD];

// acc[t][reg]: row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of the wave's 32 rows, column 32 t + (lane & 31) of its 64 columns
__device__ __forceinline__ void score_tile(const float* __restrict__ A, int na, int row0, const float* __restrict__ B, int nb, int col0, int d,
                                           SnTileRow* __restrict__ As, SnTileRow* __restrict__ Bs, f32x16 (&acc)[2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < d; k0 += SN_KC) {
    f32x4 va[2], vb[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int f = tid + i * SN_NT, rr = f >> 3, c4 = f & 7, g = row0 + rr;
      va[i] = g < na ? *reinterpret_cast<const f32x4*>(A + (int64_t)g * d + k0 + 4 * c4) : zero;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = tid + i * SN_NT, rr = f >> 3, c4 = f & 7, g = col0 + rr;
      vb[i] = g < nb ? *reinterpret_cast<const f32x4*>(B + (int64_t)g * d + k0 + 4 * c4) : zero;
    }
    __syncthreads();                                   // the previous step's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int f = tid + i * SN_NT;
      *reinterpret_cast<f32x4*>(&As[f >> 3][4 * (f & 7)]) = va[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = tid + i * SN_NT;
      *reinterpret_cast<f32x4*>(&Bs[f >> 3][4 * (f & 7)]) = vb[i];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SN_KC; kk += 8) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&As[wm * 32 + r][kk + 4 * h]);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Bs[wn * 64 + r][kk + 4 * h]);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Bs[wn * 64 + 32 + r][kk + 4 * h]);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0[s], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1[s], acc[1], 0, 0, 0);
      }
    }
  }
}

// grid (tiles of the cohort, tiles of the row block); S [nrows][M]
__global__ __launch_bounds__(SN_NT) void snorm_scores_kernel(const float* __restrict__ E, int nrows, const float* __restrict__ Cn, int M, int d,
                                                             float* __restrict__ S) {
  __shared__ __attribute__((aligned(16))) float As[SN_BM][SN_LD];
  __shared__ __attribute__((aligned(16))) float Bs[SN_BN][SN_LD];
  const int col0 = blockIdx.x * SN_BN, row0 = blockIdx.y * SN_BM;
  f32x16 acc[2];
  score_tile(E, nrows, row0, Cn, M, col0, d, As, Bs, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = col0 + wn * 64 + 32 * t + r;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = row0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (row < nrows && col < M) S[(int64_t)row * M + col] = acc[t][reg];
    }
  }
}

// larger float <-> larger key (a negative float inverts all its bits, the others set the sign bit); -0 sorts just below +0.  A NaN of either
// sign takes the largest key, so a row that holds one always selects it and its statistics are NaN
__device__ __forceinline__ uint32_t score_key(float s) {
  const uint32_t u = __float_as_uint(s);
  return s != s ? 0xffffffffu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float key_score(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

__global__ __launch_bounds__(SN_NT) void snorm_select_kernel(const float* __restrict__ S, int M, int K, float* __restrict__ mean,
                                                             float* __restrict__ sd) {
  __shared__ int s_hist[256];
  __shared__ int s_scan[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_kr;
  __shared__ double s_red[SN_NT / 64];
  const int tid = threadIdx.x;
  const float* row = S + (int64_t)blockIdx.x * M;
  uint32_t prefix = 0, mask = 0;
  int kr = K;                                          // the rank wanted among the scores whose key matches the prefix (1 = the largest)
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < M; j += SN_NT) {
      const uint32_t key = score_key(row[j]);
      if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    const int cnt = s_hist[tid];
    s_scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // s_scan[t] = the scores in the bins t .. 255
      const int v = tid + off < 256 ? s_scan[tid + off] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const int incl = s_scan[tid], above = incl - cnt;
    if (above < kr && kr <= incl) {                    // one bin holds the rank (1 <= kr <= the matching scores, as 1 <= K <= M)
      s_prefix = prefix | ((uint32_t)tid << shift);
      s_kr = kr - above;
    }
    __syncthreads();
    prefix = s_prefix;
    kr = s_kr;
    mask |= 0xffu << shift;
    __syncthreads();
  }
  // prefix = the key of the K-th largest score t; K - kr scores lie strictly above it and kr of the K are equal to t
  const uint32_t tkey = prefix;
  const double t = (double)key_score(tkey), nk = (double)kr, dK = (double)K;
  double a = 0.0;
  for (int j = tid; j < M; j += SN_NT) {
    const float s = row[j];
    if (score_key(s) > tkey) a += (double)s;
  }
  const double mu = (block_sum(a, s_red) + nk * t) / dK;
  a = 0.0;
  for (int j = tid; j < M; j += SN_NT) {
    const float s = row[j];
    if (score_key(s) > tkey) {
      const double dv = (double)s - mu;
      a += dv * dv;
    }
  }
  const double var = (block_sum(a, s_red) + nk * ((t - mu) * (t - mu))) / dK;
  if (tid == 0) {
    const float sdev = (float)sqrt(var);
    mean[blockIdx.x] = (float)mu;
    sd[blockIdx.x] = sdev < SN_STD_FLOOR ? SN_STD_FLOOR : sdev;      // a NaN stays a NaN
  }
}

// a row's best entries, best first; idx < 0: empty
struct SnTop {
  float z[SN_MAX_TOPK], raw[SN_MAX_TOPK];
  int idx[SN_MAX_TOPK];
};
__device__ __forceinline__ bool sn_better(float z, int i, float bz, int bi) { return bi < 0 || z > bz || (z == bz && i < bi); }
__device__ __forceinline__ void sn_push(SnTop& t, float z, float raw, int i) {
  if (!(z == z)) return;                               // a NaN never wins
#pragma unroll
  for (int s = 0; s < SN_MAX_TOPK; ++s) {
    if (sn_better(z, i, t.z[s], t.idx[s])) {
      const float oz = t.z[s], orw = t.raw[s];
      const int oi = t.idx[s];
      t.z[s] = z; t.raw[s] = raw; t.idx[s] = i;
      z = oz; raw = orw; i = oi;
      if (i < 0) return;
    }
  }
}

// grid = tiles of 64 windows; the workgroup walks the profile tiles.  thread = (row tid >> 2, columns 32 (tid & 3) .. + 31 of the tile)
__global__ __launch_bounds__(SN_NT) void snorm_topk_kernel(const float* __restrict__ E, const float* __restrict__ mean_e,
                                                           const float* __restrict__ std_e, int N, const float* __restrict__ P,
                                                           const float* __restrict__ mean_p, const float* __restrict__ std_p, int Pn, int d, int k,
                                                           int32_t* __restrict__ idx, float* __restrict__ score, float* __restrict__ raw) {
  __shared__ __attribute__((aligned(16))) float As[SN_BM][SN_LD];
  __shared__ __attribute__((aligned(16))) float Bs[SN_BN][SN_LD];
  __shared__ float Ss[SN_BM][SN_BN + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int row0 = blockIdx.x * SN_BM;
  const int lrow = tid >> 2, part = tid & 3, grow = row0 + lrow;
  const bool live = grow < N;
  const double me = live ? (double)mean_e[grow] : 0.0, se = live ? (double)std_e[grow] : 1.0;
  SnTop top;
#pragma unroll
  for (int s = 0; s < SN_MAX_TOPK; ++s) { top.z[s] = 0.f; top.raw[s] = 0.f; top.idx[s] = -1; }
  for (int col0 = 0; col0 < Pn; col0 += SN_BN) {
    f32x16 acc[2];
    score_tile(E, N, row0, P, Pn, col0, d, As, Bs, acc);           // its barriers also close the previous tile's reads of Ss
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) Ss[wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h][wn * 64 + 32 * t + r] = acc[t][reg];
    __syncthreads();
    if (live) {
      for (int c = part * 32; c < part * 32 + 32; ++c) {
        const int col = col0 + c;
        if (col >= Pn) break;
        const float s = Ss[lrow][c];
        const double z = 0.5 * (((double)s - me) / se + ((double)s - (double)mean_p[col]) / (double)std_p[col]);
        sn_push(top, (float)z, s, col);
      }
    }
  }
  __syncthreads();                                     // Ss becomes the lists of the four parts of every row
  float* lz = &Ss[0][0];
  float* lr = lz + SN_NT * SN_MAX_TOPK;
  int* li = reinterpret_cast<int*>(lr + SN_NT * SN_MAX_TOPK);
#pragma unroll
  for (int s = 0; s < SN_MAX_TOPK; ++s) {
    lz[tid * SN_MAX_TOPK + s] = top.z[s];
    lr[tid * SN_MAX_TOPK + s] = top.raw[s];
    li[tid * SN_MAX_TOPK + s] = top.idx[s];
  }
  __syncthreads();
  if (!live || part != 0) return;
  for (int p = 1; p < 4; ++p)
#pragma unroll
    for (int s = 0; s < SN_MAX_TOPK; ++s) {
      const int o = (tid + p) * SN_MAX_TOPK + s;
      if (li[o] >= 0) sn_push(top, lz[o], lr[o], li[o]);
    }
  const int kw = k < Pn ? k : Pn;                      // columns beyond Pn are not written
#pragma unroll
  for (int s = 0; s < SN_MAX_TOPK; ++s) {
    if (s >= kw) break;
    const bool have = top.idx[s] >= 0;
    idx[(int64_t)grow * k + s] = have ? top.idx[s] : -1;
    score[(int64_t)grow * k + s] = have ? top.z[s] : 0.f;
    raw[(int64_t)grow * k + s] = have ? top.raw[s] : 0.f;
  }
}

// the shape rules of both entry points; they come before anything that needs a device
#define SN_REQUIRE_D(fn, d) \
  SDK_REQUIRE((d) >= 64 && (d) <= SN_MAX_D && (d) % 64 == 0, fn ": d=%d not supported (a multiple of 64, at most %d)", (d), SN_MAX_D)
#define SN_REQUIRE_COHORT(fn, N, M, K)                                                                                                     \
  SDK_REQUIRE((N) >= 0 && (M) >= 1 && (M) <= SN_MAX_M && (K) >= 1 && (K) <= (M), fn ": N=%d M=%d K=%d (N at least 0, 1 <= M <= %d, 1 <= K <= M)", \
              (N), (M), (K), SN_MAX_M)

}  // namespace

extern "C" size_t sdk_cohort_stats_workspace_bytes(int N, int M, int K) {
  if (!(N >= 0 && M >= 1 && M <= SN_MAX_M && K >= 1 && K <= M)) {
    sdk_set_error("sdk_cohort_stats_workspace_bytes: N=%d M=%d K=%d (N at least 0, 1 <= M <= %d, 1 <= K <= M)", N, M, K, SN_MAX_M);
    return 0;
  }
  return ws_round((size_t)sn_alloc_rows(N, M) * (size_t)M * sizeof(float));
}

extern "C" int sdk_cohort_stats(sdk_ctx* ctx, const float* E, int N, const float* Cn, int M, int d, int K, float* mean, float* stdev, void* ws,
                                size_t ws_bytes, void* stream) {
  SN_REQUIRE_D("sdk_cohort_stats", d);
  SN_REQUIRE_COHORT("sdk_cohort_stats", N, M, K);
  SDK_REQUIRE(ctx, "sdk_cohort_stats: null context");
  if (N == 0) return 0;
  SDK_REQUIRE(E && Cn && mean && stdev && ws, "sdk_cohort_stats: null argument (E=%p Cn=%p mean=%p std=%p ws=%p)", (const void*)E, (const void*)Cn,
              (void*)mean, (void*)stdev, ws);
  SDK_REQUIRE((((uintptr_t)E | (uintptr_t)Cn | (uintptr_t)ws) & 15) == 0, "sdk_cohort_stats: E=%p, Cn=%p and ws=%p must be 16-byte aligned", (const void*)E,
              (const void*)Cn, ws);
  SDK_REQUIRE_WS("sdk_cohort_stats", "sdk_cohort_stats_workspace_bytes", ws, ws_bytes, sdk_cohort_stats_workspace_bytes(N, M, K), 1);
  const int rb = sn_alloc_rows(N, M);
  float* S = static_cast<float*>(ws);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * M * d, 4.0 * ((double)N * d + (double)ceil_div(N, rb) * M * d + 7.0 * N * M));
  for (int r0 = 0; r0 < N; r0 += rb) {
    const int rows = N - r0 < rb ? N - r0 : rb;
    hipLaunchKernelGGL(snorm_scores_kernel, dim3(ceil_div(M, SN_BN), ceil_div(rows, SN_BM)), dim3(SN_NT), 0, s, E + (int64_t)r0 * d, rows, Cn, M, d, S);
    SDK_LAUNCH_CHECK();
    if (ctx->snorm_scores_only) continue;
    hipLaunchKernelGGL(snorm_select_kernel, dim3(rows), dim3(SN_NT), 0, s, (const float*)S, M, K, mean + r0, stdev + r0);
    SDK_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int sdk_affinity_topk_snorm(sdk_ctx* ctx, const float* E, const float* mean_e, const float* std_e, int N, const float* P,
                                       const float* mean_p, const float* std_p, int Pn, int d, int k, int32_t* idx, float* score, float* raw,
                                       void* stream) {
  SN_REQUIRE_D("sdk_affinity_topk_snorm", d);
  SDK_REQUIRE(k >= 1 && k <= SN_MAX_TOPK, "sdk_affinity_topk_snorm: k=%d (1 .. %d)", k, SN_MAX_TOPK);
  SDK_REQUIRE(N >= 0 && Pn >= 1, "sdk_affinity_topk_snorm: N=%d Pn=%d (N at least 0, Pn at least 1)", N, Pn);
  SDK_REQUIRE(ctx, "sdk_affinity_topk_snorm: null context");
  if (N == 0) return 0;
  SDK_REQUIRE(E && mean_e && std_e && P && mean_p && std_p && idx && score && raw,
              "sdk_affinity_topk_snorm: null argument (E=%p mean_e=%p std_e=%p P=%p mean_p=%p std_p=%p idx=%p score=%p raw=%p)", (const void*)E,
              (const void*)mean_e, (const void*)std_e, (const void*)P, (const void*)mean_p, (const void*)std_p, (void*)idx, (void*)score, (void*)raw);
  SDK_REQUIRE((((uintptr_t)E | (uintptr_t)P) & 15) == 0, "sdk_affinity_topk_snorm: E=%p and P=%p must be 16-byte aligned", (const void*)E, (const void*)P);
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * Pn * d, 4.0 * ((double)N * d + (double)ceil_div(N, SN_BM) * Pn * d + 3.0 * N * k));
  hipLaunchKernelGGL(snorm_topk_kernel, dim3(ceil_div(N, SN_BM)), dim3(SN_NT), 0, (hipStream_t)stream, E, mean_e, std_e, N, P, mean_p, std_p, Pn, d, k,
                     idx, score, raw);
  SDK_LAUNCH_CHECK();
  return 0;
}
