// Scoring a diarization against a reference (score.py): the diarization error rate on the packed frame grid (packed_grid.hpp).
//
//   score_turns_kernel     merged reference turns [M][3] (s0, s1, speaker) -> ref_mask [G] uint64, bit i = reference speaker i active in the
//                          frame (its centre lies in [s0, s1)).  One wave per turn, a 64-bit integer atomicOr per frame of the turn.
//   score_overlap_kernel   (skip_overlap) thread = frame: scored = 0 where two or more bits are set.
//   score_collar_kernel    (collar > 0) one wave per boundary (a turn's s0 and s1): scored = 0 on the frames with |centre - b| < collar.
//   score_cooccur_kernel   ref_mask, scored, speakers [G][2] -> per recording co [S_r][K_r] int32 and tally [5] int64.  A workgroup takes
//                          SC_FRAMES consecutive packed frames and serves the recordings inside them one at a time (pg_walk): the
//                          recording's table is summed in LDS (at most 64 x 64 int32, 16 KB), then one integer atomic add per non-zero cell.
//   score_map_kernel       one wave per recording: the exact maximum-weight assignment on its co table padded with zeros to n x n,
//                          n = max(S_r, K_r) <= 64, by shortest augmenting paths with int64 potentials; column j lives on lane j and the
//                          row minimum is a cross-lane reduction.
//
// Everything is integer arithmetic.  OR, stores of one value and integer adds do not depend on the order they land in, so every output is
// bit-identical run to run; `correct` is the optimum's value, unique where the map is not.  No kernel needs an ordering between
// workgroups of one launch: the launches follow each other in stream order.
#include "common.hpp"
#include "packed_grid.hpp"

namespace {

constexpr int SC_NT = 256;
constexpr int SC_FPT = 16;                   // frames per thread of score_cooccur_kernel
constexpr int SC_FRAMES = SC_NT * SC_FPT;    // frames per workgroup

__global__ __launch_bounds__(SC_NT) void score_turns_kernel(const int32_t* __restrict__ turns, const int32_t* __restrict__ turn_off,
                                                            const int32_t* __restrict__ frame_off, const int32_t* __restrict__ ref_off, int R,
                                                            int M, unsigned long long* __restrict__ ref_mask) {
  const int t = blockIdx.x * (SC_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= M) return;
  const int r = pg_find_group(turn_off, R, t);
  const int64_t s0 = turns[3 * (int64_t)t], s1 = turns[3 * (int64_t)t + 1];
  const int i = turns[3 * (int64_t)t + 2];
  if (i < 0 || i >= ref_off[r + 1] - ref_off[r] || i >= PG_MAX_SPK || s1 <= s0) return;
  const int64_t g0 = frame_off[r], n_g = frame_off[r + 1] - g0;
  const int64_t lo = pg_first_frame(s0), hi = min(pg_first_frame(s1), n_g);      // the frames lo <= g < hi have s0 <= centre < s1
  const unsigned long long bit = 1ull << i;
  for (int64_t g = lo + lane; g < hi; g += 64) atomicOr(ref_mask + g0 + g, bit);
}

__global__ __launch_bounds__(SC_NT) void score_overlap_kernel(const unsigned long long* __restrict__ ref_mask, int G, uint8_t* __restrict__ scored) {
  const int g = blockIdx.x * SC_NT + threadIdx.x;
  if (g < G && __popcll(ref_mask[g]) >= 2) scored[g] = 0;
}

__global__ __launch_bounds__(SC_NT) void score_collar_kernel(const int32_t* __restrict__ turns, const int32_t* __restrict__ turn_off,
                                                             const int32_t* __restrict__ frame_off, int R, int M, int collar,
                                                             uint8_t* __restrict__ scored) {
  const int w = blockIdx.x * (SC_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= 2 * M) return;
  const int t = w >> 1;
  const int r = pg_find_group(turn_off, R, t);
  if (turns[3 * (int64_t)t + 1] <= turns[3 * (int64_t)t]) return;                  // no turn, no boundary
  const int64_t b = turns[3 * (int64_t)t + (w & 1)];
  const int64_t g0 = frame_off[r], n_g = frame_off[r + 1] - g0;
  const int64_t lo = pg_first_frame(b - collar + 1), hi = min(pg_first_frame(b + collar), n_g);   // b - collar < centre < b + collar
  for (int64_t g = lo + lane; g < hi; g += 64) scored[g0 + g] = 0;
}

__global__ __launch_bounds__(SC_NT) void score_cooccur_kernel(const unsigned long long* __restrict__ ref_mask, const uint8_t* __restrict__ scored,
                                                              const int32_t* __restrict__ speakers, const int32_t* __restrict__ frame_off,
                                                              const int32_t* __restrict__ ref_off, const int32_t* __restrict__ cent_off,
                                                              const int64_t* __restrict__ co_off, int R, int G, int32_t* __restrict__ co,
                                                              unsigned long long* __restrict__ tally) {
  __shared__ int32_t tab[PG_MAX_SPK * PG_MAX_SPK];
  __shared__ int32_t tal[5];
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * SC_FRAMES;
  pg_walk(frame_off, R, f0, min(f0 + SC_FRAMES, G), [&](int r, int a, int b) {
    const int S = pg_speakers(ref_off, r), K = pg_speakers(cent_off, r);
    pg_co_clear<5, SC_NT>(tab, tal, S * K);
    int n_sc = 0, n_ref = 0, n_miss = 0, n_fa = 0, n_both = 0;
    for (int g = a + tid; g < b; g += SC_NT) {
      if (!scored[g]) continue;
      unsigned long long m = ref_mask[g];
      const int h0 = speakers[2 * (int64_t)g], h1 = speakers[2 * (int64_t)g + 1];
      const int nref = __popcll(m), nhyp = (int)(h0 >= 0) + (int)(h1 >= 0);
      n_sc += 1;
      n_ref += nref;
      n_miss += max(0, nref - nhyp);
      n_fa += max(0, nhyp - nref);
      n_both += min(nref, nhyp);
      const bool on0 = h0 >= 0 && h0 < K, on1 = h1 >= 0 && h1 < K && h1 != h0;
      while (m) {
        const int i = __ffsll((long long)m) - 1;
        m &= m - 1;
        if (i >= S) break;                                      // bits ascend: nothing below S is left
        if (on0) atomicAdd(&tab[i * K + h0], 1);
        if (on1) atomicAdd(&tab[i * K + h1], 1);
      }
    }
    pg_co_flush<5, SC_NT>(tab, tal, {n_sc, n_ref, n_miss, n_fa, n_both}, S * K, co + co_off[r], tally + 5 * (int64_t)r);
  });
}

struct ScKey { long long v; int j; };
__device__ __forceinline__ ScKey sc_wave_argmin(long long v, int j) {             // least v, ties to the least j
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ov = __shfl_xor(v, o, 64);
    const int oj = __shfl_xor(j, o, 64);
    if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; }
  }
  return {v, j};
}

// Shortest augmenting paths on cost = -co, rows entered one at a time (the Hungarian method in its potentials form).  Lane j holds column
// j's potential v, the row matched to it, and the search's minv / way / used; the rows' potentials u sit in LDS.  The dummy column that the
// search starts from is the uniform pair (j0 == -1, row i).
__global__ __launch_bounds__(64) void score_map_kernel(const int32_t* __restrict__ co, const int32_t* __restrict__ ref_off,
                                                       const int32_t* __restrict__ cent_off, const int64_t* __restrict__ co_off,
                                                       int32_t* __restrict__ map, long long* __restrict__ correct) {
  __shared__ int32_t w[PG_MAX_SPK * PG_MAX_SPK];
  __shared__ long long u[PG_MAX_SPK];
  __shared__ int32_t row_col[PG_MAX_SPK];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int S = pg_speakers(ref_off, r), K = pg_speakers(cent_off, r);
  const int n = max(S, K);
  if (n <= 0) {
    if (lane == 0) correct[r] = 0;
    return;
  }
  const int32_t* src = co + co_off[r];
  for (int c = lane; c < n * PG_MAX_SPK; c += 64) {
    const int i = c >> 6, j = c & 63;
    w[c] = (i < S && j < K) ? src[i * K + j] : 0;
  }
  u[lane] = 0;
  row_col[lane] = -1;
  __syncthreads();
  constexpr long long INF = 1ll << 62;
  long long v = 0;
  int p = -1;                                                   // the row matched to this lane's column
  for (int i = 0; i < n; ++i) {
    long long minv = INF;
    int way = -1;
    bool used = lane >= n;                                      // columns past n never enter
    int j0 = -1, i0 = i;
    for (;;) {
      const long long ui0 = u[i0];
      if (!used) {
        const long long cur = -(long long)w[i0 * PG_MAX_SPK + lane] - ui0 - v;
        if (cur < minv) { minv = cur; way = j0; }
      }
      const ScKey best = sc_wave_argmin(used ? INF : minv, lane);
      const long long delta = best.v;
      __syncthreads();                                          // every lane has read u[i0]
      if (used && lane < n) { u[p] += delta; v -= delta; }      // used columns are matched to pairwise different rows
      else if (!used) minv -= delta;
      if (lane == 0) u[i] += delta;                             // the dummy column's row: not matched yet, so no used column names it
      __syncthreads();
      j0 = best.j;
      if (lane == j0) used = true;
      i0 = __shfl(p, j0, 64);
      if (i0 < 0) break;                                        // a free column: the path ends
    }
    while (j0 >= 0) {                                           // flip the path back to the dummy column
      const int j1 = __shfl(way, j0, 64);
      const int pj1 = j1 >= 0 ? __shfl(p, j1 & 63, 64) : i;
      if (lane == j0) p = pj1;
      j0 = j1;
    }
  }
  long long sum = 0;
  if (lane < K && p >= 0 && p < S) {
    const int c = w[p * PG_MAX_SPK + lane];
    if (c > 0) { row_col[p] = lane; sum = c; }                  // a pair that never co-occurs is no pair
  }
  sum = wave_sum(sum);
  __syncthreads();
  if (lane < S) map[ref_off[r] + lane] = row_col[lane];
  if (lane == 0) correct[r] = sum;
}

}  // namespace

extern "C" int sdk_score_reference(sdk_ctx* ctx, const int32_t* turns, const int32_t* turn_off, const int32_t* frame_off, const int32_t* ref_off, int R,
                                   int M, int64_t G, int max_ref, int collar, int skip_overlap, uint64_t* ref_mask, uint8_t* scored, void* stream) {
  SDK_REQUIRE(ctx, "sdk_score_reference: null context");
  SDK_REQUIRE(R >= 1 && M >= 0 && G >= 0 && G < (1ll << 30) && M < (1 << 28), "sdk_score_reference: R=%d M=%d G=%lld (R at least 1, fewer than 2^28 turns and 2^30 frames)",
              R, M, (long long)G);
  SDK_REQUIRE(max_ref >= 0 && max_ref <= PG_MAX_SPK, "sdk_score_reference: %d reference speakers in a recording (at most %d)", max_ref, PG_MAX_SPK);
  SDK_REQUIRE(collar >= 0 && collar < (1 << 30) && (skip_overlap == 0 || skip_overlap == 1), "sdk_score_reference: collar=%d samples (0 .. 2^30 - 1), skip_overlap=%d (0 or 1)",
              collar, skip_overlap);
  if (G == 0) return 0;
  SDK_REQUIRE(frame_off && ref_mask && scored && (M == 0 || (turns && turn_off && ref_off)), "sdk_score_reference: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 9.0 * G + 12.0 * M);
  SDK_HIP_OK(hipMemsetAsync(ref_mask, 0, (size_t)G * 8, s));
  SDK_HIP_OK(hipMemsetAsync(scored, 1, (size_t)G, s));
  if (M) {
    hipLaunchKernelGGL(score_turns_kernel, pg_grid(M, SC_NT / 64), dim3(SC_NT), 0, s, turns, turn_off, frame_off, ref_off, R, M, (unsigned long long*)ref_mask);
    SDK_LAUNCH_CHECK();
  }
  if (skip_overlap && M) {
    hipLaunchKernelGGL(score_overlap_kernel, pg_grid(G, SC_NT), dim3(SC_NT), 0, s, (const unsigned long long*)ref_mask, (int)G, scored);
    SDK_LAUNCH_CHECK();
  }
  if (collar > 0 && M) {
    hipLaunchKernelGGL(score_collar_kernel, pg_grid(2 * (int64_t)M, SC_NT / 64), dim3(SC_NT), 0, s, turns, turn_off, frame_off, R, M, collar, scored);
    SDK_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int sdk_score_cooccur(sdk_ctx* ctx, const uint64_t* ref_mask, const uint8_t* scored, const int32_t* speakers, const int32_t* frame_off,
                                 const int32_t* ref_off, const int32_t* cent_off, const int64_t* co_off, int R, int64_t G, int max_ref, int max_hyp,
                                 int64_t co_total, int32_t* co, int64_t* tally, void* stream) {
  SDK_REQUIRE(ctx, "sdk_score_cooccur: null context");
  SDK_REQUIRE(R >= 1 && G >= 0 && G < (1ll << 30) && co_total >= 0, "sdk_score_cooccur: R=%d G=%lld co_total=%lld (R at least 1, fewer than 2^30 frames)", R,
              (long long)G, (long long)co_total);
  SDK_REQUIRE(max_ref >= 0 && max_ref <= PG_MAX_SPK && max_hyp >= 0 && max_hyp <= PG_MAX_SPK,
              "sdk_score_cooccur: %d reference and %d hypothesis speakers in a recording (at most %d each)", max_ref, max_hyp, PG_MAX_SPK);
  SDK_REQUIRE(tally && (co_total == 0 || co), "sdk_score_cooccur: null argument (co=%p tally=%p)", (void*)co, (void*)tally);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 17.0 * G + 4.0 * co_total);
  SDK_HIP_OK(hipMemsetAsync(tally, 0, (size_t)R * 5 * 8, s));
  if (co_total) SDK_HIP_OK(hipMemsetAsync(co, 0, (size_t)co_total * 4, s));
  if (G == 0) return 0;
  SDK_REQUIRE(ref_mask && scored && speakers && frame_off && ref_off && cent_off && co_off, "sdk_score_cooccur: null argument");
  hipLaunchKernelGGL(score_cooccur_kernel, pg_grid(G, SC_FRAMES), dim3(SC_NT), 0, s, (const unsigned long long*)ref_mask, scored, speakers, frame_off, ref_off,
                     cent_off, co_off, R, (int)G, co, (unsigned long long*)tally);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_score_map(sdk_ctx* ctx, const int32_t* co, const int32_t* ref_off, const int32_t* cent_off, const int64_t* co_off, int R, int max_ref,
                             int max_hyp, int32_t* map, int64_t* correct, void* stream) {
  SDK_REQUIRE(ctx, "sdk_score_map: null context");
  SDK_REQUIRE(R >= 1, "sdk_score_map: R=%d (at least 1)", R);
  SDK_REQUIRE(max_ref >= 0 && max_ref <= PG_MAX_SPK && max_hyp >= 0 && max_hyp <= PG_MAX_SPK,
              "sdk_score_map: %d reference and %d hypothesis speakers in a recording (at most %d each)", max_ref, max_hyp, PG_MAX_SPK);
  SDK_REQUIRE(ref_off && cent_off && co_off && correct && (max_ref == 0 || map) && (max_ref == 0 || max_hyp == 0 || co), "sdk_score_map: null argument");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)R * (4.0 * max_ref * max_hyp + 4.0 * max_ref + 8.0));
  hipLaunchKernelGGL(score_map_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, co, ref_off, cent_off, co_off, map, (long long*)correct);
  SDK_LAUNCH_CHECK();
  return 0;
}
