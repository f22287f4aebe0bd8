// AS-norm verification trials: every (test row, model row) pair scored on the cohort-normalised scale, classed and binned - neither the score
// matrix nor the normalised one is written (trials_snorm.py states the rule; trials, classes, exclusions, q, a pass and the counters are those
// of trials.hip).
//
//   s(i, j) = sum_k A[i][k] B[j][k]                                               float64, tr_hist_kernel's chain (no r)
//   z(i, j) = ((s - mean_a[i]) * inv_a[i] + (s - mean_b[j]) * inv_b[j]) * 0.5     six rounded float64 operations in this order: subtract,
//                                                                                 multiply, subtract, multiply, add, multiply - never an FMA
//   t = (z - lo) * scale, then q, bin and the counters exactly as in tr_hist_kernel; a NaN z is counted in nan[class].
//   inv = 1 / std is formed by the caller (one division per ROW): a trial costs no division.
//
//   tr_hist_snorm_kernel tr_hist_kernel's design with its own copy of the tile product (trials.hip says why the product is not shared):
//                        persistent workgroups over contiguous runs of 64 x 64 tiles, model tiles fastest; four waves, each a 32 x 32 quadrant =
//                        2 x 2 v_mfma_f64_16x16x4_f64 tiles; A and B through LDS in chunks of 16 columns, the next chunk in flight in registers
//                        during the MFMAs (two stages: registers, then LDS); rows outside the matrices staged as zeros and NOT counted; in-range
//                        trials by ONE LDS integer atomic into hist[class][bin], under / over / nan / excluded in per-lane registers; flushed
//                        with 64-bit integer global atomics at the end and at least every TS_FLUSH_TILES tiles.
//                        The four statistics of a tile travel like its labels: threads 0 .. 63 load the test rows' (mean, inv), threads
//                        64 .. 127 the model rows', only for rows inside the matrices (the aok / bok guard: a row past N or M is never
//                        dereferenced), written to LDS after the tile's first barrier, read in the epilogue.  2 KB of LDS more than
//                        tr_hist_kernel without its r: 55 KB, two workgroups per CU.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage: 109 VGPRs + 32 AGPRs (tr_hist_kernel: 101 + 32), 106 SGPRs of which 12 are
// kept in VGPR lanes (tr_hist_kernel: 8), no scratch, 56320 bytes of LDS, 2 waves per SIMD (the LDS binds: two workgroups per CU).  The
// epilogue compiles to 128 float64 VALU operations per lane and tile (16 trials x 8: the six of z and the two of t) and no v_fma_f64.
//
// Measured (tools/snorm_trials_bench.py, profiles/r32_snorm_trials_bench.json): N = M = 65 536: 45.9 ms at K = 192 and 56.2 ms at K = 256 beside
// tr_hist_kernel's 44.7 and 54.7 ms on the same rows in the same run (2.8 % and 2.7 % more; 2.6 % and 2.7 % at 16 384 rows): 46 % and 50 % of the
// 78.6 TFLOP/s fp64 matrix peak.  The same z as a bilinear form of width 400 through tr_hist_kernel takes 1.69 x as long.  Not tuned.
//
// The file is compiled with -ffp-contract=off (Makefile): the z chain must keep its six roundings, and the compiler may otherwise contract the
// second product with the addition.  The MFMAs are builtins and are not affected.
// Everything after z is integer arithmetic; integer atomics commute: the counters do not depend on the grid, the tile order or the arrival
// order, and two runs agree bit for bit.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int TS_NT = 256;
constexpr int TS_BM = 64, TS_BN = 64;       // tile of the workgroup: test rows x model rows
constexpr int TS_KC = 16;                   // columns k staged per step
constexpr int TS_LD = 80;                   // LDS row pitch in doubles (as trials.hip)
constexpr int TS_BINS = 4096;
constexpr int TS_Q_BITS = 24;
constexpr int TS_MAX_ROWS = 1 << 20;
constexpr int TS_MAX_K = 512;
constexpr int TS_DEFAULT_BLOCKS = 512;      // 256 CUs x 2 workgroups (55 KB of LDS each)
constexpr int TS_FLUSH_TILES = 1 << 19;     // tiles between two flushes of the LDS histogram
constexpr int TS_OUT = 2 * TS_BINS + 7;     // hist[2][4096], under[2], over[2], nan[2], excluded[1]
constexpr int TS_LDS_BYTES = 2 * TS_KC * TS_LD * 8 + 2 * TS_BINS * 4 + 4 * 64 * 4 + 4 * 64 * 8;

static_assert((uint64_t)TS_FLUSH_TILES * (uint64_t)(TS_BM * TS_BN) <= 0xffffffffull, "a uint32 counter cannot wrap between two flushes");
static_assert(TS_LDS_BYTES <= 65536, "static LDS of the kernel");
static_assert(2 * TS_LDS_BYTES <= 160 * 1024, "two workgroups per CU");

typedef double ts_d4 __attribute__((ext_vector_type(4)));
typedef double ts_d2 __attribute__((ext_vector_type(2)));

struct TsCount {
  uint32_t under[2], over[2], nan[2], excluded;
};

__global__ __launch_bounds__(TS_NT) void tr_hist_snorm_kernel(const double* __restrict__ A, int N, const double* __restrict__ B, int M, int K,
                                                              const double* __restrict__ mean_a, const double* __restrict__ inv_a,
                                                              const double* __restrict__ mean_b, const double* __restrict__ inv_b,
                                                              const int32_t* __restrict__ la, const int32_t* __restrict__ sa,
                                                              const int32_t* __restrict__ lb, const int32_t* __restrict__ sb, double lo,
                                                              double scale, int shift, uint32_t base, int ntn, int ntiles,
                                                              unsigned long long* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double s_mem[2 * TS_KC * TS_LD];
  __shared__ uint32_t s_hist[2 * TS_BINS];
  __shared__ int32_t s_la[TS_BM], s_sa[TS_BM], s_lb[TS_BN], s_sb[TS_BN];
  __shared__ double s_ma[TS_BM], s_ia[TS_BM], s_mb[TS_BN], s_ib[TS_BN];
  double (*s_a)[TS_LD] = reinterpret_cast<double (*)[TS_LD]>(s_mem);                      // [TS_KC][TS_LD]: A[row][k] as [k][row]
  double (*s_b)[TS_LD] = reinterpret_cast<double (*)[TS_LD]>(s_mem + TS_KC * TS_LD);      // [TS_KC][TS_LD]: B[row][k] as [k][row]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = wave >> 1, qj = wave & 1, fk = lane >> 4, fc = lane & 15;
  // staging: thread = (row tid & 63 of the tile, columns 4 (tid >> 6) .. + 3 of the chunk)
  const int sr = tid & 63, sk = 4 * (tid >> 6);
  const int t0 = (int)((int64_t)blockIdx.x * ntiles / gridDim.x), t1 = (int)((int64_t)(blockIdx.x + 1) * ntiles / gridDim.x);
  for (int i = tid; i < 2 * TS_BINS; i += TS_NT) s_hist[i] = 0;       // before the first tile's barriers
  TsCount c = {{0, 0}, {0, 0}, {0, 0}, 0};
  const ts_d2 zero2 = {0.0, 0.0};

  auto flush = [&]() {                                                // every wave's epilogue is done (a barrier precedes)
    for (int i = tid; i < 2 * TS_BINS; i += TS_NT) {
      const uint32_t v = s_hist[i];
      if (v) {
        atomicAdd(out + i, (unsigned long long)v);
        s_hist[i] = 0;
      }
    }
    uint32_t v[7] = {c.under[0], c.under[1], c.over[0], c.over[1], c.nan[0], c.nan[1], c.excluded};
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = wave_sum(v[k]);             // at most 64 lanes x 2^19 tiles x 16 elements = 2^29
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (v[k]) atomicAdd(out + 2 * TS_BINS + k, (unsigned long long)v[k]);
    }
    c = TsCount{{0, 0}, {0, 0}, {0, 0}, 0};
  };

  int since = 0;
  for (int tile = t0; tile < t1; ++tile) {
    const int row0 = (tile / ntn) * TS_BM, col0 = (tile % ntn) * TS_BN;
    const int64_t arow = row0 + sr, brow = col0 + sr;
    const bool aok = arow < N, bok = brow < M;
    ts_d2 ra[2], rb[2];
    auto fetch = [&](int d0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ra[h] = aok ? *reinterpret_cast<const ts_d2*>(A + arow * K + d0 + sk + 2 * h) : zero2;
        rb[h] = bok ? *reinterpret_cast<const ts_d2*>(B + brow * K + d0 + sk + 2 * h) : zero2;
      }
    };
    ts_d4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = ts_d4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    // the tile's labels, sessions and statistics: written after the first barrier (the previous tile's epilogue has read its own), read in the
    // epilogue; a row outside the matrices is not dereferenced and its slots are never read (the epilogue skips it)
    int32_t my_l = -1, my_s = -1;
    double my_m = 0.0, my_i = 0.0;
    if (tid < 64) {
      if (aok) { my_l = la[arow]; my_s = sa[arow]; my_m = mean_a[arow]; my_i = inv_a[arow]; }
    } else if (tid < 128) {
      if (bok) { my_l = lb[brow]; my_s = sb[brow]; my_m = mean_b[brow]; my_i = inv_b[brow]; }
    }
    for (int d0 = 0; d0 < K; d0 += TS_KC) {
      __syncthreads();                                   // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          s_a[sk + 2 * h + e][sr] = ra[h][e];
          s_b[sk + 2 * h + e][sr] = rb[h][e];
        }
      if (d0 == 0) {
        if (tid < 64) { s_la[sr] = my_l; s_sa[sr] = my_s; s_ma[sr] = my_m; s_ia[sr] = my_i; }
        else if (tid < 128) { s_lb[sr] = my_l; s_sb[sr] = my_s; s_mb[sr] = my_m; s_ib[sr] = my_i; }
      }
      __syncthreads();
      if (d0 + TS_KC < K) fetch(d0 + TS_KC);             // in flight during the MFMAs
#pragma unroll
      for (int ks = 0; ks < TS_KC / 4; ++ks) {
        const int kk = ks * 4 + fk;
        const double a0 = s_a[kk][qi * 32 + fc], a1 = s_a[kk][qi * 32 + 16 + fc];
        const double b0 = s_b[kk][qj * 32 + fc], b1 = s_b[kk][qj * 32 + 16 + fc];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg.  Labels and statistics were written before this tile's last barrier.
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int lc = qj * 32 + v * 16 + fc;
      const bool cok = col0 + lc < M;
      const int32_t lbj = s_lb[lc], sbj = s_sb[lc];
      const double mbj = s_mb[lc], ibj = s_ib[lc];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lr = qi * 32 + u * 16 + fk + 4 * reg;
          if (!cok || row0 + lr >= N) continue;          // outside the matrices: not a trial
          const int32_t lai = s_la[lr], sai = s_sa[lr];
          if (lai < 0 || lbj < 0 || (sai >= 0 && sai == sbj)) {
            c.excluded += 1;
            continue;
          }
          const int cls = lai == lbj ? 1 : 0;
          const double s = acc[u][v][reg];
          const double za = __dmul_rn(__dsub_rn(s, s_ma[lr]), s_ia[lr]);
          const double zb = __dmul_rn(__dsub_rn(s, mbj), ibj);
          const double z = __dmul_rn(__dadd_rn(za, zb), 0.5);
          const double t = __dmul_rn(__dsub_rn(z, lo), scale);
          if (t != t) {
            c.nan[cls] += 1;
          } else if (t < 0.0) {
            c.under[cls] += 1;
          } else if (t >= 16777216.0) {
            c.over[cls] += 1;
          } else {
            const uint32_t qs = (uint32_t)t >> shift;    // t in [0, 2^24): the conversion truncates = floor
            if (qs < base) {
              c.under[cls] += 1;
            } else if (qs - base >= (uint32_t)TS_BINS) {
              c.over[cls] += 1;
            } else {
              atomicAdd(&s_hist[cls * TS_BINS + (int)(qs - base)], 1u);
            }
          }
        }
    }
    if (++since == TS_FLUSH_TILES) {
      __syncthreads();
      flush();
      since = 0;
    }
  }
  __syncthreads();
  flush();
}

}  // namespace

extern "C" int sdk_trial_hist_snorm(sdk_ctx* ctx, const double* A, int N, const double* B, int M, int K, const double* mean_a, const double* inv_a,
                                    const double* mean_b, const double* inv_b, const int32_t* la, const int32_t* sa, const int32_t* lb,
                                    const int32_t* sb, double lo, double scale, int shift, int base, int max_blocks, uint64_t* out, void* stream) {
  SDK_REQUIRE(K >= 16 && K <= TS_MAX_K && K % 16 == 0, "sdk_trial_hist_snorm: K=%d not supported (a multiple of 16 in 16 .. %d)", K, TS_MAX_K);
  SDK_REQUIRE(N >= 1 && N <= TS_MAX_ROWS && M >= 1 && M <= TS_MAX_ROWS, "sdk_trial_hist_snorm: N=%d test rows, M=%d model rows (1 .. %d each)", N, M,
              TS_MAX_ROWS);
  SDK_REQUIRE(shift >= 0 && shift <= TS_Q_BITS, "sdk_trial_hist_snorm: shift=%d (0 .. %d)", shift, TS_Q_BITS);
  SDK_REQUIRE(base >= 0 && base <= (1 << TS_Q_BITS), "sdk_trial_hist_snorm: base=%d (0 .. 2^%d)", base, TS_Q_BITS);
  SDK_REQUIRE(max_blocks >= 0, "sdk_trial_hist_snorm: max_blocks=%d (0: the default grid, else a cap on the workgroups)", max_blocks);
  SDK_REQUIRE(lo > -INFINITY && lo < INFINITY && scale > 0.0 && scale < INFINITY,
              "sdk_trial_hist_snorm: lo=%g scale=%g (lo finite, scale = 2^24 / (hi - lo) finite and above 0: lo < hi)", lo, scale);
  SDK_REQUIRE(ctx, "sdk_trial_hist_snorm: null context");
  SDK_REQUIRE(A && B && mean_a && inv_a && mean_b && inv_b && la && sa && lb && sb && out,
              "sdk_trial_hist_snorm: null argument (A=%p B=%p mean_a=%p inv_a=%p mean_b=%p inv_b=%p la=%p sa=%p lb=%p sb=%p out=%p)", (const void*)A,
              (const void*)B, (const void*)mean_a, (const void*)inv_a, (const void*)mean_b, (const void*)inv_b, (const void*)la, (const void*)sa,
              (const void*)lb, (const void*)sb, (void*)out);
  SDK_REQUIRE((((uintptr_t)A | (uintptr_t)B) & 15) == 0, "sdk_trial_hist_snorm: A=%p and B=%p must be 16-byte aligned", (const void*)A, (const void*)B);
  SDK_REQUIRE((((uintptr_t)out | (uintptr_t)mean_a | (uintptr_t)inv_a | (uintptr_t)mean_b | (uintptr_t)inv_b) & 7) == 0,
              "sdk_trial_hist_snorm: out=%p and the four statistics must be 8-byte aligned", (void*)out);
  const int ntm = ceil_div(N, TS_BM), ntn = ceil_div(M, TS_BN);
  const int64_t tiles = (int64_t)ntm * ntn;              // at most 2^28
  int grid = tiles < TS_DEFAULT_BLOCKS ? (int)tiles : TS_DEFAULT_BLOCKS;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * (double)M * K, 8.0 * (double)tiles * (TS_BM + TS_BN) * K);
  SDK_HIP_OK(hipMemsetAsync(out, 0, (size_t)TS_OUT * sizeof(uint64_t), st));
  hipLaunchKernelGGL(tr_hist_snorm_kernel, dim3(grid), dim3(TS_NT), 0, st, A, N, B, M, K, mean_a, inv_a, mean_b, inv_b, la, sa, lb, sb, lo, scale,
                     shift, (uint32_t)base, ntn, (int)tiles, reinterpret_cast<unsigned long long*>(out));
  SDK_LAUNCH_CHECK();
  return 0;
}
