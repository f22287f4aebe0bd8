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
//   tr_hist_snorm_kernel tt_walk, trial_bin and tt_flush of trial_tile.hpp (the walk over the tiles, the product, the classes and exclusions, the
//                        histogram and its flush are tr_hist_kernel's, written once there).  The payload of a row is its (mean, inv), on both
//                        sides: threads 0 .. 63 load the test rows', threads 64 .. 127 the model rows', only for rows inside the matrices (a
//                        row past N or M is never dereferenced), written to LDS after the tile's first barrier, read in the epilogue.  2 KB of
//                        LDS more than tr_hist_kernel without its r: 55 KB, two workgroups per CU.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage: 118 VGPRs + 32 AGPRs (109 when the kernel had its own copy of the
// walk; tr_hist_kernel: 95 + 32), 106 SGPRs, no scratch, 56320 bytes of LDS, 2 waves per SIMD (the LDS binds: two workgroups per CU).  The
// compiled kernel has no v_fma_f64.
//
// Measured with its own copy of the walk (tools/snorm_trials_bench.py, profiles/r32_snorm_trials_bench.json): N = M = 65 536: 45.9 ms at
// K = 192 and 56.2 ms at K = 256 beside tr_hist_kernel's 44.7 and 54.7 ms on the same rows in the same run (2.8 % and 2.7 % more; 2.6 % and
// 2.7 % at 16 384 rows): 46 % and 50 % of the 78.6 TFLOP/s fp64 matrix peak.  The same z as a bilinear form of width 400 through
// tr_hist_kernel takes 1.69 x as long.  Not tuned.  On the shared walk (profiles/r36_trial_tile_ab.json, medians of three runs each, copy ->
// shared): 46.07 -> 45.17 ms and 56.51 -> 55.41 ms.
//
// The file is compiled with -ffp-contract=off (Makefile): the z chain must keep its six roundings, and the compiler may otherwise contract the
// second product with the addition.  The MFMAs are builtins and are not affected.
// Everything after z is integer arithmetic; integer atomics commute: the counters do not depend on the grid, the tile order or the arrival
// order, and two runs agree bit for bit.
#include "trial_tile.hpp"

namespace {

constexpr int TS_LDS_BYTES = TT_HIST_LDS_BYTES + 4 * 64 * 8;
static_assert(TS_LDS_BYTES <= 65536, "static LDS of the kernel");
static_assert(2 * TS_LDS_BYTES <= 160 * 1024, "two workgroups per CU");

__global__ __launch_bounds__(TT_NT) void tr_hist_snorm_kernel(const double* __restrict__ A, int N, const double* __restrict__ B, int M, int K,
                                                              const double* __restrict__ mean_a, const double* __restrict__ inv_a,
                                                              const double* __restrict__ mean_b, const double* __restrict__ inv_b,
                                                              const int32_t* __restrict__ la, const int32_t* __restrict__ sa,
                                                              const int32_t* __restrict__ lb, const int32_t* __restrict__ sb, double lo,
                                                              double scale, int shift, uint32_t base, int ntn, int ntiles,
                                                              unsigned long long* __restrict__ out) {
  __shared__ TtTile s_tile;
  __shared__ uint32_t s_hist[2 * TT_BINS];
  __shared__ double s_ma[TT_BM], s_ia[TT_BM], s_mb[TT_BN], s_ib[TT_BN];
  tt_hist_clear(s_hist);
  TtCount c = {{0, 0}, {0, 0}, {0, 0}, 0, {0, 0}};
  int since = 0;
  tt_walk<tt_d2>(
      TtMatrices{A, B, la, sa, lb, sb, N, M, K, ntn, ntiles}, s_tile, c.excluded,
      [&](bool model, int64_t row) { return model ? tt_d2{mean_b[row], inv_b[row]} : tt_d2{mean_a[row], inv_a[row]}; },
      [&](bool model, int lr, tt_d2 p) {
        if (model) { s_mb[lr] = p[0]; s_ib[lr] = p[1]; }
        else { s_ma[lr] = p[0]; s_ia[lr] = p[1]; }
      },
      [&](int lc) { return tt_d2{s_mb[lc], s_ib[lc]}; },
      [&](int cls, double s, int lr, int lc, tt_d2 bj) {
        const double za = __dmul_rn(__dsub_rn(s, s_ma[lr]), s_ia[lr]);
        const double zb = __dmul_rn(__dsub_rn(s, bj[0]), bj[1]);
        const double z = __dmul_rn(__dadd_rn(za, zb), 0.5);
        trial_bin(__dmul_rn(__dsub_rn(z, lo), scale), cls, shift, base, s_hist, c);
      },
      [&]() { tt_flush_due(since, s_hist, c, out); });
  __syncthreads();
  tt_flush(s_hist, c, out);
}

}  // namespace

extern "C" int sdk_trial_hist_snorm(sdk_ctx* ctx, const double* A, int N, const double* B, int M, int K, const double* mean_a, const double* inv_a,
                                    const double* mean_b, const double* inv_b, const int32_t* la, const int32_t* sa, const int32_t* lb,
                                    const int32_t* sb, double lo, double scale, int shift, int base, int max_blocks, uint64_t* out, void* stream) {
  if (int rc = tt_require_range("sdk_trial_hist_snorm", lo, scale, shift, base)) return rc;
  if (int rc = tt_require("sdk_trial_hist_snorm", ctx, N, M, K, max_blocks,
                          {{"A", A}, {"B", B}, {"mean_a", mean_a}, {"inv_a", inv_a}, {"mean_b", mean_b}, {"inv_b", inv_b}, {"la", la}, {"sa", sa},
                           {"lb", lb}, {"sb", sb}, {"out", out}}))
    return rc;
  SDK_REQUIRE((((uintptr_t)out | (uintptr_t)mean_a | (uintptr_t)inv_a | (uintptr_t)mean_b | (uintptr_t)inv_b) & 7) == 0,
              "sdk_trial_hist_snorm: out=%p and the four statistics must be 8-byte aligned", (void*)out);
  int64_t tiles = 0;
  const int grid = tt_grid(N, M, max_blocks, &tiles), ntn = ceil_div(M, TT_BN);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * (double)M * K, 8.0 * (double)tiles * (TT_BM + TT_BN) * K);
  SDK_HIP_OK(hipMemsetAsync(out, 0, (size_t)TT_OUT * sizeof(uint64_t), st));
  hipLaunchKernelGGL(tr_hist_snorm_kernel, dim3(grid), dim3(TT_NT), 0, st, A, N, B, M, K, mean_a, inv_a, mean_b, inv_b, la, sa, lb, sb, lo, scale,
                     shift, (uint32_t)base, ntn, (int)tiles, reinterpret_cast<unsigned long long*>(out));
  SDK_LAUNCH_CHECK();
  return 0;
}
