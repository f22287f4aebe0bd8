// Verification trials: every (test row, model row) pair scored, classed and binned - the score matrix is never written (trials.py states the rule).
//
//   s(i, j) = r[j] + sum_k A[i][k] B[j][k]   float64;   t = (s - lo) * scale (one subtraction, one multiplication, never an FMA);
//   q, bin, classes, exclusions, the walk over the tiles, the product and the flush: trial_tile.hpp, which the three trial kernels share.
//
//   tr_hist_kernel       tt_walk with r[j] as the model rows' payload; the epilogue adds r after the product, forms t and bins it (trial_bin).
//
// Everything after the product is integer arithmetic; integer atomics commute: the counters do not depend on the grid, the tile order or the
// arrival order, and two runs agree bit for bit.  The product itself is one chain in one order per element, as in ps_score_kernel.
//
// The walk was three copies (here twice, trials_snorm.hip once) until it was measured shared.  hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage, copies -> shared: tr_hist_kernel<false> 103 -> 98 VGPRs, tr_hist_kernel<true> 101 -> 95,
// tr_calib_kernel 191 -> 186; 32 AGPRs, 106 SGPRs, no scratch, the same LDS (54784 / 22528 bytes) and 2 waves per SIMD before and after.
// Times (profiles/r36_trial_tile_ab.json, medians of three runs each, N = M = 65 536, K = 192 / 256, copies -> shared): trial_hist pass 1
// 44.88 -> 44.78 / 55.09 -> 54.84 ms, the calibration pass 69.04 -> 68.99 / 78.52 -> 78.40 ms; DESIGN.md has the rest.
#include "trial_tile.hpp"

namespace {

static_assert(TT_HIST_LDS_BYTES + 64 * 8 <= 65536, "static LDS of the kernel");

// HIST = false: the bench-only variant without the LDS atomics (in-range trials are counted per class in a register and land in bin 0)
template <bool HIST>
__global__ __launch_bounds__(TT_NT) void tr_hist_kernel(const double* __restrict__ A, int N, const double* __restrict__ B,
                                                        const double* __restrict__ r, int M, int K, const int32_t* __restrict__ la,
                                                        const int32_t* __restrict__ sa, const int32_t* __restrict__ lb,
                                                        const int32_t* __restrict__ sb, double lo, double scale, int shift, uint32_t base,
                                                        int ntn, int ntiles, unsigned long long* __restrict__ out) {
  __shared__ TtTile s_tile;
  __shared__ uint32_t s_hist[2 * TT_BINS];
  __shared__ double s_r[TT_BN];
  tt_hist_clear(s_hist);
  TtCount c = {{0, 0}, {0, 0}, {0, 0}, 0, {0, 0}};
  int since = 0;
  tt_walk<double>(
      TtMatrices{A, B, la, sa, lb, sb, N, M, K, ntn, ntiles}, s_tile, c.excluded,
      [&](bool model, int64_t row) { return model ? r[row] : 0.0; },
      [&](bool model, int lr, double p) {
        if (model) s_r[lr] = p;
      },
      [&](int lc) { return s_r[lc]; },
      [&](int cls, double acc, int lr, int lc, double rj) {
        const double s = acc + rj;
        trial_bin<HIST>(__dmul_rn(__dsub_rn(s, lo), scale), cls, shift, base, s_hist, c);
      },
      [&]() { tt_flush_due<HIST>(since, s_hist, c, out); });
  __syncthreads();
  tt_flush<HIST>(s_hist, c, out);
}

// ---- calibration: the sums of the logistic objective over every trial (trials.py states the rule) -----------------------------------------------
//
//   tr_calib_kernel      tt_walk with the same payload; the epilogue, on the accumulator registers, forms per trial
//                          z = a * s + c (one multiplication, one addition, never an FMA), m = +z (target) or -z, e = exp(-|m|),
//                          loss = max(-m, 0) + log1p(e), p = e / (1 + e), q = 1 / (1 + e), w = p (m >= 0) or q, v = p * q
//                        and adds the seven terms loss, w, w s, v, v s, (v s) s, s into the lane's sums of the trial's class (the other class
//                        gets + 0.0, which changes nothing: no divergent copy of the additions).  A score that is not finite is counted and left
//                        out.  No histogram: 22 KB of LDS.
//                        Reduction, without a float atomic: a lane's chain runs in tile order (16 trials of a tile in register order); at the end
//                        a fixed xor tree over the 64 lanes (offsets 32, 16, .. 1), the four waves through LDS added in wave order, ONE row
//                        [2][8] per workgroup in `partials` (slot 0 of a class: its count, a uint64; slots 1 .. 7: the sums).  nonfinite and
//                        excluded are integers and go to `counts` with 64-bit integer atomics, as in tr_hist_kernel.
//   tr_calib_sum_kernel  one workgroup: adds the rows in ascending block order.
// The sums are a function of the inputs and the grid alone: two runs agree bit for bit; another max_blocks changes the order of the additions.
constexpr int TC_TERMS = 7;                 // loss, w, w s, v, v s, v s^2, s
constexpr int TC_ROW = 2 * (TC_TERMS + 1);  // a workgroup's row of partials: [2][8]
constexpr int TC_COUNTS = 5;                // n[2], nonfinite[2], excluded
// the default grid is two workgroups per CU: the registers bind, not the LDS (forced to 3 waves / SIMD the kernel fits 168 VGPRs with 12 bytes of
// scratch per lane: not taken, unmeasured)

__global__ __launch_bounds__(TT_NT) void tr_calib_kernel(const double* __restrict__ A, int N, const double* __restrict__ B,
                                                         const double* __restrict__ r, int M, int K, const int32_t* __restrict__ la,
                                                         const int32_t* __restrict__ sa, const int32_t* __restrict__ lb,
                                                         const int32_t* __restrict__ sb, double ca, double cc, int ntn, int ntiles,
                                                         double* __restrict__ partials, unsigned long long* __restrict__ counts) {
  __shared__ TtTile s_tile;
  __shared__ double s_r[TT_BN];
  __shared__ double s_red[4][2 * TC_TERMS];
  __shared__ unsigned long long s_cnt[4][2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double sum[2][TC_TERMS];
#pragma unroll
  for (int k = 0; k < TC_TERMS; ++k) sum[0][k] = sum[1][k] = 0.0;
  unsigned long long n[2] = {0, 0}, nonfinite[2] = {0, 0}, excluded = 0;      // 64 bits: one workgroup may own all 2^28 tiles
  tt_walk<double>(
      TtMatrices{A, B, la, sa, lb, sb, N, M, K, ntn, ntiles}, s_tile, excluded,
      [&](bool model, int64_t row) { return model ? r[row] : 0.0; },
      [&](bool model, int lr, double p) {
        if (model) s_r[lr] = p;
      },
      [&](int lc) { return s_r[lc]; },
      [&](int cls, double acc, int lr, int lc, double rj) {
        const bool tgt = cls == 1;
        const double s = acc + rj;
        if (!(fabs(s) < INFINITY)) {                     // NaN, +inf, -inf
          nonfinite[tgt ? 1 : 0] += 1;
          return;
        }
        const double z = __dadd_rn(__dmul_rn(ca, s), cc);
        const double m = tgt ? z : -z;
        const double e = exp(-fabs(m));
        const double d = __dadd_rn(1.0, e);
        const double p = e / d, q = 1.0 / d;
        const double w = m >= 0.0 ? p : q;
        const double hv = __dmul_rn(p, q), hs = __dmul_rn(hv, s);
        const double term[TC_TERMS] = {__dadd_rn(fmax(-m, 0.0), log1p(e)), w, __dmul_rn(w, s), hv, hs, __dmul_rn(hs, s), s};
#pragma unroll
        for (int k = 0; k < TC_TERMS; ++k) {
          sum[0][k] = __dadd_rn(sum[0][k], tgt ? 0.0 : term[k]);
          sum[1][k] = __dadd_rn(sum[1][k], tgt ? term[k] : 0.0);
        }
        n[0] += tgt ? 0 : 1;
        n[1] += tgt ? 1 : 0;
      },
      []() {});
  // the lanes of a wave, then the waves, then one row per workgroup
#pragma unroll
  for (int c = 0; c < 2; ++c) {
#pragma unroll
    for (int k = 0; k < TC_TERMS; ++k) {
      const double t = wave_sum(sum[c][k]);
      if (lane == 0) s_red[wave][c * TC_TERMS + k] = t;
    }
    const unsigned long long tn = wave_sum(n[c]), tf = wave_sum(nonfinite[c]);
    if (lane == 0) {
      s_cnt[wave][c] = tn;
      if (tf) atomicAdd(counts + 2 + c, tf);
    }
  }
  const unsigned long long tx = wave_sum(excluded);
  if (lane == 0 && tx) atomicAdd(counts + 4, tx);
  __syncthreads();
  double* row = partials + (size_t)blockIdx.x * TC_ROW;
  if (tid < 2 * TC_TERMS) {
    const double t = __dadd_rn(__dadd_rn(__dadd_rn(s_red[0][tid], s_red[1][tid]), s_red[2][tid]), s_red[3][tid]);
    row[(tid / TC_TERMS) * (TC_TERMS + 1) + 1 + tid % TC_TERMS] = t;
  } else if (tid < 2 * TC_TERMS + 2) {
    const int c = tid - 2 * TC_TERMS;
    reinterpret_cast<unsigned long long*>(row)[c * (TC_TERMS + 1)] = s_cnt[0][c] + s_cnt[1][c] + s_cnt[2][c] + s_cnt[3][c];
  }
}

// one workgroup of 64: thread t < 16 owns slot t of the row [2][8] and adds the workgroups' rows in ascending order
__global__ __launch_bounds__(64) void tr_calib_sum_kernel(const double* __restrict__ partials, int rows, double* __restrict__ sums,
                                                          unsigned long long* __restrict__ counts) {
  const int t = threadIdx.x;
  if (t >= TC_ROW) return;
  const int c = t / (TC_TERMS + 1), k = t % (TC_TERMS + 1);
  if (k == 0) {
    unsigned long long v = 0;
    for (int b = 0; b < rows; ++b) v += reinterpret_cast<const unsigned long long*>(partials)[(size_t)b * TC_ROW + t];
    counts[c] = v;
  } else {
    double v = 0.0;
    for (int b = 0; b < rows; ++b) v = __dadd_rn(v, partials[(size_t)b * TC_ROW + t]);
    sums[c * TC_TERMS + k - 1] = v;
  }
}

}  // namespace

extern "C" int sdk_trial_hist(sdk_ctx* ctx, const double* A, int N, const double* B, const double* r, int M, int K, const int32_t* la,
                              const int32_t* sa, const int32_t* lb, const int32_t* sb, double lo, double scale, int shift, int base, int max_blocks,
                              uint64_t* out, void* stream) {
  if (int rc = tt_require_range("sdk_trial_hist", lo, scale, shift, base)) return rc;
  if (int rc = tt_require("sdk_trial_hist", ctx, N, M, K, max_blocks,
                          {{"A", A}, {"B", B}, {"r", r}, {"la", la}, {"sa", sa}, {"lb", lb}, {"sb", sb}, {"out", out}}))
    return rc;
  SDK_REQUIRE(((uintptr_t)out & 7) == 0, "sdk_trial_hist: out=%p must be 8-byte aligned", (void*)out);
  int64_t tiles = 0;
  const int grid = tt_grid(N, M, max_blocks, &tiles), ntn = ceil_div(M, TT_BN);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * (double)M * K, 8.0 * (double)tiles * (TT_BM + TT_BN) * K);
  SDK_HIP_OK(hipMemsetAsync(out, 0, (size_t)TT_OUT * sizeof(uint64_t), st));
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  if (ctx->trials_no_hist)
    hipLaunchKernelGGL(tr_hist_kernel<false>, dim3(grid), dim3(TT_NT), 0, st, A, N, B, r, M, K, la, sa, lb, sb, lo, scale, shift, (uint32_t)base, ntn,
                       (int)tiles, o);
  else
    hipLaunchKernelGGL(tr_hist_kernel<true>, dim3(grid), dim3(TT_NT), 0, st, A, N, B, r, M, K, la, sa, lb, sb, lo, scale, shift, (uint32_t)base, ntn,
                       (int)tiles, o);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t sdk_trial_calib_workspace_bytes(int N, int M, int max_blocks) {
  if (!(N >= 1 && N <= TT_MAX_ROWS && M >= 1 && M <= TT_MAX_ROWS && max_blocks >= 0)) {
    sdk_set_error("sdk_trial_calib_workspace_bytes: N=%d M=%d max_blocks=%d (1 <= N, M <= %d, max_blocks at least 0)", N, M, max_blocks, TT_MAX_ROWS);
    return 0;
  }
  return ws_round((size_t)tt_grid(N, M, max_blocks, nullptr) * TC_ROW * sizeof(double));
}

extern "C" int sdk_trial_calib(sdk_ctx* ctx, const double* A, int N, const double* B, const double* r, int M, int K, const int32_t* la,
                               const int32_t* sa, const int32_t* lb, const int32_t* sb, double a, double c, int max_blocks, double* sums,
                               uint64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(a > -INFINITY && a < INFINITY && c > -INFINITY && c < INFINITY, "sdk_trial_calib: a=%g c=%g (the map z = a s + c: both finite)", a, c);
  if (int rc = tt_require("sdk_trial_calib", ctx, N, M, K, max_blocks,
                          {{"A", A}, {"B", B}, {"r", r}, {"la", la}, {"sa", sa}, {"lb", lb}, {"sb", sb}, {"sums", sums}, {"counts", counts}}))
    return rc;
  SDK_REQUIRE((((uintptr_t)sums | (uintptr_t)counts) & 7) == 0, "sdk_trial_calib: sums=%p and counts=%p must be 8-byte aligned", (void*)sums,
              (void*)counts);
  int64_t tiles = 0;
  const int grid = tt_grid(N, M, max_blocks, &tiles);
  SDK_REQUIRE_WS("sdk_trial_calib", "sdk_trial_calib_workspace_bytes", ws, ws_bytes, (size_t)grid * TC_ROW * sizeof(double), 256);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * (double)M * K, 8.0 * (double)tiles * (TT_BM + TT_BN) * K);
  SDK_HIP_OK(hipMemsetAsync(counts, 0, (size_t)TC_COUNTS * sizeof(uint64_t), st));
  double* partials = static_cast<double*>(ws);
  unsigned long long* cn = reinterpret_cast<unsigned long long*>(counts);
  hipLaunchKernelGGL(tr_calib_kernel, dim3(grid), dim3(TT_NT), 0, st, A, N, B, r, M, K, la, sa, lb, sb, a, c, ceil_div(M, TT_BN), (int)tiles, partials,
                     cn);
  SDK_LAUNCH_CHECK();
  hipLaunchKernelGGL(tr_calib_sum_kernel, dim3(1), dim3(64), 0, st, partials, grid, sums, cn);
  SDK_LAUNCH_CHECK();
  return 0;
}
