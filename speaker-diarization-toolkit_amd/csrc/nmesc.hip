// The nearest-neighbour graph of eigengap spectral clustering (cluster.nmesc_cluster, clustering="nmesc"; the rule is stated in cluster.py):
// the neighbour lists of unit rows, their reverse (incoming) edges as CSR, the degrees of the graph pruned to p neighbours, and the lazy
// normalised operator T_p = (I + D^-1/2 A_p D^-1/2) / 2 applied to a thin block.
//
//   knn_reset_kernel      status = {0, INT_MAX} (sdk_knn_rows_fused: twice)
//   knn_finite_kernel     wave = one row: a non-finite value counts the row in status[0] and lowers status[1] to it (integer atomics)
//   knn_rows_kernel       workgroup = KNN_RB = 32 query rows, wave = KNN_RW = 8 of them, lane = one candidate row of the current tile of
//                         KNN_TC = 64 candidates.  The candidates' columns pass through LDS transposed, in tiles of KNN_TJ = 64 columns, beside
//                         the query rows' columns, both as float64; a lane runs one fma chain per query row over the columns in ascending
//                         order (fp32 x fp32 is exact in float64, so the chain IS the sum of exact products, rounded once per addition).
//                         Selection: each query row's list lives in the wave's registers, lane l holding its l-th best (cosine, row); a
//                         ballot finds the tile's candidates that beat the list's last entry, and each of those is inserted by a
//                         popcount of the entries ahead of it and one shift up.  After the first tiles few candidates pass the ballot
//                         (about P ln(n / P) insertions per row in all), so the selection stays far below the product.
//   knn_map_range_kernel  thread = one map entry of sdk_knn_rows_fused: an entry outside [0, n_all) counts in status[2] and lowers status[3] to its base row
//   knn_finite_ref_kernel wave = one row of E_all: a row with a non-finite value that some map entry names (the wave then scans the maps, which
//                         happens for such rows only) counts in status[0] and lowers status[1] to it
//   knn_rows_fused_kernel knn_rows_kernel's schedule on GATHERED rows (the multi-scale affinity of cluster.nmesc_multiscale): per tile of
//                         candidates and per scale s the rows maps[s][.] pass through the same LDS images, the same chains (knn_tile_fma) give
//                         c_s, and f = f + w_s c_s (one rounded product, one rounded addition) runs over the scales in order before the one
//                         shared selection (knn_select_tile).  8 more float64 accumulators per lane than knn_rows_kernel, the same LDS.
//   knn_count_kernel      thread = one list entry: the count of (source chunk of KNN_CH = 256 rows, target) pairs, integer atomics
//   knn_scan_chunks_kernel thread = one target: its counts over the chunks turned into exclusive prefix sums, the total to tot[]
//   knn_scan_rows_kernel  one workgroup: rev_off = the exclusive prefix sums of tot[] (a segment per thread, the segments' sums in thread order)
//   knn_fill_kernel       wave = one chunk: its source rows one after another, lane = rank.  The targets of one row are distinct, so within
//                         a step every cursor has one writer, and the steps of a chunk follow each other in the one wave that owns its
//                         cursors: entry (source, rank) lands at rev_off[target] + the sources below it that list target, whatever the
//                         schedule.
//   knn_degree_kernel     wave = one row: deg = p + the reverse entries of rank < p, dinv = 1 / sqrt(deg) (two rounded float64 operations)
//   knn_matvec_kernel     thread = (row, column): the float64 sum over the out-neighbours by rank, then over the reverse entries in stored
//                         order, every product and every addition rounded on its own (__dmul_rn, __dadd_rn: no contraction)
//
// No floating-point atomics; every output element has one owner; the integer atomics count, and a count does not depend on the order of its
// increments: two runs agree bit for bit.
#include "common.hpp"

#include <climits>

namespace {

constexpr int KNN_NT = 256;
constexpr int KNN_P_MAX = 64;        // one lane per list entry (cluster.NMESC_P_MAX)
constexpr int KNN_MAX_D = 512;
constexpr int KNN_MAX_ROWS = 65536;
constexpr int KNN_RB = 32;           // query rows per workgroup
constexpr int KNN_RW = KNN_RB / 4;   // query rows per wave
constexpr int KNN_TC = 64;           // candidate rows per tile: one lane each
constexpr int KNN_TJ = 64;           // columns per LDS tile
constexpr int KNN_CH = 256;          // source rows per chunk of the reverse fill
constexpr int KNN_MAX_KV = 32;       // the widest block of the mat-vec (THIN_MAX)
constexpr int KNN_MAX_SCALES = 8;    // the scales of sdk_knn_rows_fused (wav.BUCKETS_S holds four)

struct KnnWeights { double v[KNN_MAX_SCALES]; };       // by value in the kernel's arguments: read with scalar loads, no device copy

struct KnnWs {
  int32_t* cnt;      // [ceil(n / KNN_CH)][n] reverse-edge counts per chunk of source rows
  int32_t* tot;      // [n]
};
size_t knn_carve(WsCarver c, int n, KnnWs* w) {
  const size_t nch = (size_t)(n + KNN_CH - 1) / KNN_CH;
  w->cnt = c.take<int32_t>(nch * n);
  w->tot = c.take<int32_t>(n);
  return c.bytes();
}

bool knn_shape_ok(int n, int P) { return n >= 2 && n <= KNN_MAX_ROWS && P == (n - 1 < KNN_P_MAX ? n - 1 : KNN_P_MAX); }

__global__ __launch_bounds__(64) void knn_reset_kernel(int32_t* __restrict__ status, int pairs) {
  if ((int)threadIdx.x < pairs) { status[2 * threadIdx.x] = 0; status[2 * threadIdx.x + 1] = INT_MAX; }
}

__global__ __launch_bounds__(KNN_NT) void knn_finite_kernel(const float* __restrict__ E, int n, int d, int32_t* __restrict__ status) {
  const int t = blockIdx.x * (KNN_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= n) return;                                  // uniform over the wave
  const float* e = E + (int64_t)t * d;
  bool bad = false;
  for (int j = lane; j < d; j += 64) bad |= !isfinite(e[j]);
  if (__ballot(bad) != 0 && lane == 0) { atomicAdd(&status[0], 1); atomicMin(&status[1], t); }
}

// (cosine, row): the larger cosine first, ties to the lower row; row == INT_MAX: an empty entry, behind everything
__device__ __forceinline__ bool knn_ahead(double v, int j, double lv, int lj) { return j != INT_MAX && (lj == INT_MAX || v > lv || (v == lv && j < lj)); }

// one column tile of the chains: lane = candidate row, acc[q] += the wave's q-th query row's columns times the candidate's, in column order
__device__ __forceinline__ void knn_tile_fma(const double (*s_c)[KNN_TC + 1], const double (*s_e)[KNN_TJ], int wave, int lane, double (&acc)[KNN_RW]) {
#pragma unroll 4
  for (int jj = 0; jj < KNN_TJ; ++jj) {
    const double c = s_c[jj][lane];
#pragma unroll
    for (int q = 0; q < KNN_RW; ++q) acc[q] = fma(s_e[wave * KNN_RW + q][jj], c, acc[q]);
  }
}

// the selection both list kernels share: val[q] is the value of (query row t0 + wave KNN_RW + q, candidate row j0 + lane); each query row's
// list lives in the wave's registers, lane l holding its l-th best (value, row)
__device__ __forceinline__ void knn_select_tile(const double (&val)[KNN_RW], double (&lv)[KNN_RW], int (&lj)[KNN_RW], int t0, int wave, int lane, int j0,
                                                int n, int P) {
  const int j = j0 + lane;
#pragma unroll
  for (int q = 0; q < KNN_RW; ++q) {
    const int t = t0 + wave * KNN_RW + q;
    if (t >= n) break;                                 // uniform over the wave
    // a NaN value (a non-finite row: the call's status names it) ranks as -inf and is stored as that
    const double v = val[q] == val[q] ? val[q] : -INFINITY;
    const int cj = (j < n && j != t) ? j : INT_MAX;
    double tv = __shfl(lv[q], P - 1, 64);
    int tj = __shfl(lj[q], P - 1, 64);
    unsigned long long mask = __ballot(knn_ahead(v, cj, tv, tj));
    while (mask) {                                     // uniform: the candidates of this tile in lane (= row) order
      const int b = __ffsll((long long)mask) - 1;
      const double bv = __shfl(v, b, 64);
      const int bj = __shfl(cj, b, 64);
      const bool behind = knn_ahead(bv, bj, lv[q], lj[q]);            // this entry comes after the candidate: a suffix of the list
      const int pos = __popcll(~__ballot(behind));
      const double uv = __shfl_up(lv[q], 1, 64);
      const int uj = __shfl_up(lj[q], 1, 64);
      if (lane == pos) { lv[q] = bv; lj[q] = bj; }
      else if (lane > pos) { lv[q] = uv; lj[q] = uj; }
      tv = __shfl(lv[q], P - 1, 64);
      tj = __shfl(lj[q], P - 1, 64);
      const unsigned long long above = b == 63 ? 0ull : ~((2ull << b) - 1ull);
      mask = __ballot(knn_ahead(v, cj, tv, tj)) & above;
    }
  }
}

__device__ __forceinline__ void knn_store_lists(const double (&lv)[KNN_RW], const int (&lj)[KNN_RW], int t0, int wave, int lane, int n, int P,
                                                int32_t* __restrict__ idx, double* __restrict__ cosv) {
#pragma unroll
  for (int q = 0; q < KNN_RW; ++q) {
    const int t = t0 + wave * KNN_RW + q;
    if (t < n && lane < P) {
      idx[(int64_t)t * P + lane] = lj[q];
      cosv[(int64_t)t * P + lane] = lv[q];
    }
  }
}

__global__ __launch_bounds__(KNN_NT) void knn_rows_kernel(const float* __restrict__ E, int n, int d, int P, int32_t* __restrict__ idx,
                                                          double* __restrict__ cosv) {
  __shared__ double s_c[KNN_TJ][KNN_TC + 1];           // 33 KB: a tile of the candidates' columns, transposed (+1: the transposing stores spread over the banks)
  __shared__ double s_e[KNN_RB][KNN_TJ];               // 16 KB: the same columns of the workgroup's query rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, t0 = blockIdx.x * KNN_RB;
  double lv[KNN_RW];
  int lj[KNN_RW];
#pragma unroll
  for (int q = 0; q < KNN_RW; ++q) { lv[q] = 0.0; lj[q] = INT_MAX; }
  for (int j0 = 0; j0 < n; j0 += KNN_TC) {
    double acc[KNN_RW];
#pragma unroll
    for (int q = 0; q < KNN_RW; ++q) acc[q] = 0.0;
    for (int c0 = 0; c0 < d; c0 += KNN_TJ) {
      __syncthreads();
      for (int i = tid; i < KNN_TC * KNN_TJ; i += KNN_NT) {
        const int r = i / KNN_TJ, c = i - r * KNN_TJ, j = j0 + r;
        s_c[c][r] = j < n ? (double)E[(int64_t)j * d + c0 + c] : 0.0;
      }
      for (int i = tid; i < KNN_RB * KNN_TJ; i += KNN_NT) {
        const int r = i / KNN_TJ, c = i - r * KNN_TJ, t = t0 + r;
        s_e[r][c] = t < n ? (double)E[(int64_t)t * d + c0 + c] : 0.0;
      }
      __syncthreads();
      knn_tile_fma(s_c, s_e, wave, lane, acc);
    }
    knn_select_tile(acc, lv, lj, t0, wave, lane, j0, n, P);
  }
  knn_store_lists(lv, lj, t0, wave, lane, n, P, idx, cosv);
}

__global__ __launch_bounds__(KNN_NT) void knn_map_range_kernel(const int32_t* __restrict__ maps, int S, int n, int n_all, int32_t* __restrict__ status) {
  const int e = blockIdx.x * KNN_NT + threadIdx.x;     // S n <= 8 * 65536
  if (e >= S * n) return;
  if ((unsigned)maps[e] >= (unsigned)n_all) { atomicAdd(&status[2], 1); atomicMin(&status[3], e % n); }
}

__global__ __launch_bounds__(KNN_NT) void knn_finite_ref_kernel(const float* __restrict__ E, int n_all, int d, const int32_t* __restrict__ maps, int m,
                                                                int32_t* __restrict__ status) {
  const int t = blockIdx.x * (KNN_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= n_all) return;                              // uniform over the wave
  const float* e = E + (int64_t)t * d;
  bool bad = false;
  for (int j = lane; j < d; j += 64) bad |= !isfinite(e[j]);
  if (__ballot(bad) == 0) return;
  bool named = false;                                  // a non-finite row: does a map entry name it?
  for (int e0 = 0; e0 < m && !named; e0 += 64) named = __ballot(e0 + lane < m && maps[e0 + lane] == t) != 0;
  if (named && lane == 0) { atomicAdd(&status[0], 1); atomicMin(&status[1], t); }
}

__global__ __launch_bounds__(KNN_NT) void knn_rows_fused_kernel(const float* __restrict__ E, int n_all, int d, const int32_t* __restrict__ maps,
                                                                const KnnWeights w, int S, int n, int P, int32_t* __restrict__ idx,
                                                                double* __restrict__ cosv) {
  __shared__ double s_c[KNN_TJ][KNN_TC + 1];           // knn_rows_kernel's two images, filled through the maps
  __shared__ double s_e[KNN_RB][KNN_TJ];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, t0 = blockIdx.x * KNN_RB;
  double lv[KNN_RW];
  int lj[KNN_RW];
#pragma unroll
  for (int q = 0; q < KNN_RW; ++q) { lv[q] = 0.0; lj[q] = INT_MAX; }
  for (int j0 = 0; j0 < n; j0 += KNN_TC) {
    double f[KNN_RW];
#pragma unroll
    for (int q = 0; q < KNN_RW; ++q) f[q] = 0.0;
    for (int s = 0; s < S; ++s) {
      const int32_t* map = maps + (int64_t)s * n;
      double acc[KNN_RW];
#pragma unroll
      for (int q = 0; q < KNN_RW; ++q) acc[q] = 0.0;
      for (int c0 = 0; c0 < d; c0 += KNN_TJ) {
        __syncthreads();
        // r is uniform over a wave (KNN_TJ = 64 consecutive i share it): the map entry is one broadcast load.  An entry that is not a row
        // of E_all (the call's status counts it) gathers nothing: its columns are zeros.
        for (int i = tid; i < KNN_TC * KNN_TJ; i += KNN_NT) {
          const int r = i / KNN_TJ, c = i - r * KNN_TJ, j = j0 + r;
          const int g = j < n ? map[j] : -1;
          s_c[c][r] = (unsigned)g < (unsigned)n_all ? (double)E[(int64_t)g * d + c0 + c] : 0.0;
        }
        for (int i = tid; i < KNN_RB * KNN_TJ; i += KNN_NT) {
          const int r = i / KNN_TJ, c = i - r * KNN_TJ, t = t0 + r;
          const int g = t < n ? map[t] : -1;
          s_e[r][c] = (unsigned)g < (unsigned)n_all ? (double)E[(int64_t)g * d + c0 + c] : 0.0;
        }
        __syncthreads();
        knn_tile_fma(s_c, s_e, wave, lane, acc);
      }
      const double ws = w.v[s];
#pragma unroll
      for (int q = 0; q < KNN_RW; ++q) f[q] = __dadd_rn(f[q], __dmul_rn(ws, acc[q]));
    }
    knn_select_tile(f, lv, lj, t0, wave, lane, j0, n, P);
  }
  knn_store_lists(lv, lj, t0, wave, lane, n, P, idx, cosv);
}

__global__ __launch_bounds__(KNN_NT) void knn_count_kernel(const int32_t* __restrict__ idx, int n, int P, int32_t* __restrict__ cnt,
                                                           int32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * KNN_NT + threadIdx.x;
  if (e >= (int64_t)n * P) return;
  const int i = (int)(e / P), j = idx[e];
  if ((unsigned)j >= (unsigned)n) { atomicAdd(&status[0], 1); atomicMin(&status[1], i); return; }
  atomicAdd(&cnt[(int64_t)(i / KNN_CH) * n + j], 1);
}

__global__ __launch_bounds__(KNN_NT) void knn_scan_chunks_kernel(int n, int nch, int32_t* __restrict__ cnt, int32_t* __restrict__ tot) {
  const int j = blockIdx.x * KNN_NT + threadIdx.x;
  if (j >= n) return;
  int run = 0;
  for (int c = 0; c < nch; ++c) {
    const int v = cnt[(int64_t)c * n + j];
    cnt[(int64_t)c * n + j] = run;
    run += v;
  }
  tot[j] = run;
}

__global__ __launch_bounds__(KNN_NT) void knn_scan_rows_kernel(int n, const int32_t* __restrict__ tot, int32_t* __restrict__ rev_off) {
  __shared__ int s_part[KNN_NT];
  const int tid = threadIdx.x, seg = (n + KNN_NT - 1) / KNN_NT, a = min(n, tid * seg), b = min(n, a + seg);
  int sum = 0;
  for (int j = a; j < b; ++j) sum += tot[j];
  s_part[tid] = sum;
  __syncthreads();
  int run = 0;
  for (int q = 0; q < tid; ++q) run += s_part[q];
  for (int j = a; j < b; ++j) { rev_off[j] = run; run += tot[j]; }
  if (tid == KNN_NT - 1) rev_off[n] = run;
}

__global__ __launch_bounds__(64) void knn_fill_kernel(const int32_t* __restrict__ idx, int n, int P, const int32_t* __restrict__ rev_off,
                                                      int32_t* __restrict__ cnt, int32_t* __restrict__ rev_src, int32_t* __restrict__ rev_rank) {
  const int ch = blockIdx.x, lane = threadIdx.x, i0 = ch * KNN_CH, i1 = min(n, i0 + KNN_CH);
  int32_t* cur = cnt + (int64_t)ch * n;
  for (int i = i0; i < i1; ++i) {
    if (lane < P) {
      const int j = idx[(int64_t)i * P + lane];
      if ((unsigned)j < (unsigned)n) {
        const int pos = rev_off[j] + atomicAdd(&cur[j], 1);        // one writer per cursor in this step; the next step waits for the value
        rev_src[pos] = i;
        rev_rank[pos] = lane;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(KNN_NT) void knn_degree_kernel(const int32_t* __restrict__ rev_off, const int32_t* __restrict__ rev_rank, int n, int p,
                                                            int32_t* __restrict__ deg, double* __restrict__ dinv) {
  const int i = blockIdx.x * (KNN_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;                                  // uniform over the wave
  int c = 0;
  for (int e = rev_off[i] + lane; e < rev_off[i + 1]; e += 64) c += rev_rank[e] < p;
  c = wave_sum(c);
  if (lane == 0) {
    deg[i] = p + c;
    dinv[i] = __ddiv_rn(1.0, __dsqrt_rn((double)(p + c)));
  }
}

__global__ __launch_bounds__(KNN_NT) void knn_matvec_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ rev_off,
                                                            const int32_t* __restrict__ rev_src, const int32_t* __restrict__ rev_rank,
                                                            const double* __restrict__ dinv, int n, int P, int p, const float* __restrict__ X, int kv,
                                                            float* __restrict__ Y) {
  const int64_t t = (int64_t)blockIdx.x * KNN_NT + threadIdx.x;
  if (t >= (int64_t)n * kv) return;
  const int i = (int)(t / kv), c = (int)(t - (int64_t)i * kv);
  double s = 0.0;
  const int32_t* li = idx + (int64_t)i * P;
#pragma unroll 4
  for (int r = 0; r < p; ++r) {
    const int j = li[r];
    if ((unsigned)j >= (unsigned)n) continue;          // not a row (sdk_knn_reverse's status names it): skipped, as there
    s = __dadd_rn(s, __dmul_rn(dinv[j], (double)X[(int64_t)j * kv + c]));
  }
  const int e1 = rev_off[i + 1];
#pragma unroll 4
  for (int e = rev_off[i]; e < e1; ++e) {
    if (rev_rank[e] >= p) continue;
    const int j = rev_src[e];
    if ((unsigned)j >= (unsigned)n) continue;
    s = __dadd_rn(s, __dmul_rn(dinv[j], (double)X[(int64_t)j * kv + c]));
  }
  Y[t] = (float)__dmul_rn(0.5, __dadd_rn((double)X[t], __dmul_rn(dinv[i], s)));
}

}  // namespace

extern "C" int sdk_knn_rows(sdk_ctx* ctx, const float* E, int n, int d, int P, int32_t* idx, double* cosv, int32_t* status, void* stream) {
  SDK_REQUIRE(ctx, "sdk_knn_rows: null context");
  SDK_REQUIRE(n >= 2 && n <= KNN_MAX_ROWS, "sdk_knn_rows: n=%d (2 .. %d)", n, KNN_MAX_ROWS);
  SDK_REQUIRE(d >= 64 && d <= KNN_MAX_D && d % 64 == 0, "sdk_knn_rows: d=%d not supported (a multiple of 64, at most %d)", d, KNN_MAX_D);
  SDK_REQUIRE(knn_shape_ok(n, P), "sdk_knn_rows: P=%d must be min(%d, n - 1) (n=%d)", P, KNN_P_MAX, n);
  SDK_REQUIRE(E && idx && cosv && status, "sdk_knn_rows: null argument (E=%p idx=%p cos=%p status=%p)", (const void*)E, (void*)idx, (void*)cosv,
              (void*)status);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * (double)n * n * d, (double)n * (4.0 * d + 12.0 * P));
  hipLaunchKernelGGL(knn_reset_kernel, dim3(1), dim3(64), 0, st, status, 1);
  hipLaunchKernelGGL(knn_finite_kernel, dim3((n + 3) / 4), dim3(KNN_NT), 0, st, E, n, d, status);
  hipLaunchKernelGGL(knn_rows_kernel, dim3((n + KNN_RB - 1) / KNN_RB), dim3(KNN_NT), 0, st, E, n, d, P, idx, cosv);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_knn_rows_fused(sdk_ctx* ctx, const float* E_all, int n_all, int d, const int32_t* maps, const double* weights, int S, int n, int P,
                                  int32_t* idx, double* cosv, int32_t* status, void* stream) {
  SDK_REQUIRE(ctx, "sdk_knn_rows_fused: null context");
  SDK_REQUIRE(S >= 1 && S <= KNN_MAX_SCALES, "sdk_knn_rows_fused: S=%d scales (1 .. %d)", S, KNN_MAX_SCALES);
  SDK_REQUIRE(n >= 2 && n <= KNN_MAX_ROWS, "sdk_knn_rows_fused: n=%d (2 .. %d)", n, KNN_MAX_ROWS);
  SDK_REQUIRE(n_all >= 1 && n_all <= KNN_MAX_SCALES * KNN_MAX_ROWS, "sdk_knn_rows_fused: n_all=%d (1 .. %d)", n_all, KNN_MAX_SCALES * KNN_MAX_ROWS);
  SDK_REQUIRE(d >= 64 && d <= KNN_MAX_D && d % 64 == 0, "sdk_knn_rows_fused: d=%d not supported (a multiple of 64, at most %d)", d, KNN_MAX_D);
  SDK_REQUIRE(knn_shape_ok(n, P), "sdk_knn_rows_fused: P=%d must be min(%d, n - 1) (n=%d)", P, KNN_P_MAX, n);
  SDK_REQUIRE(E_all && maps && weights && idx && cosv && status,
              "sdk_knn_rows_fused: null argument (E_all=%p maps=%p weights=%p idx=%p cos=%p status=%p)", (const void*)E_all, (const void*)maps,
              (const void*)weights, (void*)idx, (void*)cosv, (void*)status);
  KnnWeights w = {};
  for (int s = 0; s < S; ++s) w.v[s] = weights[s];     // host memory: the weights travel in the kernel's arguments
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * (double)S * n * n * d, (double)S * n * (4.0 * d + 4.0) + 12.0 * (double)n * P);
  hipLaunchKernelGGL(knn_reset_kernel, dim3(1), dim3(64), 0, st, status, 2);
  hipLaunchKernelGGL(knn_map_range_kernel, dim3((S * n + KNN_NT - 1) / KNN_NT), dim3(KNN_NT), 0, st, maps, S, n, n_all, status);
  hipLaunchKernelGGL(knn_finite_ref_kernel, dim3((n_all + 3) / 4), dim3(KNN_NT), 0, st, E_all, n_all, d, maps, S * n, status);
  hipLaunchKernelGGL(knn_rows_fused_kernel, dim3((n + KNN_RB - 1) / KNN_RB), dim3(KNN_NT), 0, st, E_all, n_all, d, maps, w, S, n, P, idx, cosv);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t sdk_knn_reverse_workspace_bytes(int n, int P) {
  if (!knn_shape_ok(n, P)) {
    sdk_set_error("sdk_knn_reverse_workspace_bytes: n=%d P=%d (n 2 .. %d, P = min(%d, n - 1))", n, P, KNN_MAX_ROWS, KNN_P_MAX);
    return 0;
  }
  KnnWs w;
  return knn_carve({}, n, &w);
}

extern "C" int sdk_knn_reverse(sdk_ctx* ctx, const int32_t* idx, int n, int P, int32_t* rev_off, int32_t* rev_src, int32_t* rev_rank,
                               int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx, "sdk_knn_reverse: null context");
  SDK_REQUIRE(knn_shape_ok(n, P), "sdk_knn_reverse: n=%d P=%d (n 2 .. %d, P = min(%d, n - 1))", n, P, KNN_MAX_ROWS, KNN_P_MAX);
  SDK_REQUIRE(idx && rev_off && rev_src && rev_rank && status && ws, "sdk_knn_reverse: null argument (idx=%p rev_off=%p rev_src=%p rev_rank=%p status=%p ws=%p)",
              (const void*)idx, (void*)rev_off, (void*)rev_src, (void*)rev_rank, (void*)status, ws);
  SDK_REQUIRE_WS("sdk_knn_reverse", "sdk_knn_reverse_workspace_bytes", ws, ws_bytes, sdk_knn_reverse_workspace_bytes(n, P), 256);
  const int nch = (n + KNN_CH - 1) / KNN_CH;
  KnnWs w;
  knn_carve({static_cast<char*>(ws), 0}, n, &w);
  int32_t *const cnt = w.cnt, *const tot = w.tot;
  const size_t cnt_bytes = ws_round((size_t)nch * n * sizeof(int32_t));
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 16.0 * (double)n * P + 8.0 * (double)nch * n);
  SDK_HIP_OK(hipMemsetAsync(cnt, 0, cnt_bytes, st));
  hipLaunchKernelGGL(knn_reset_kernel, dim3(1), dim3(64), 0, st, status, 1);
  const int64_t m = (int64_t)n * P;
  hipLaunchKernelGGL(knn_count_kernel, dim3((unsigned)((m + KNN_NT - 1) / KNN_NT)), dim3(KNN_NT), 0, st, idx, n, P, cnt, status);
  hipLaunchKernelGGL(knn_scan_chunks_kernel, dim3((n + KNN_NT - 1) / KNN_NT), dim3(KNN_NT), 0, st, n, nch, cnt, tot);
  hipLaunchKernelGGL(knn_scan_rows_kernel, dim3(1), dim3(KNN_NT), 0, st, n, tot, rev_off);
  hipLaunchKernelGGL(knn_fill_kernel, dim3(nch), dim3(64), 0, st, idx, n, P, rev_off, cnt, rev_src, rev_rank);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_knn_degree(sdk_ctx* ctx, const int32_t* rev_off, const int32_t* rev_rank, int n, int P, int p, int32_t* deg, double* dinv,
                              void* stream) {
  SDK_REQUIRE(ctx, "sdk_knn_degree: null context");
  SDK_REQUIRE(knn_shape_ok(n, P), "sdk_knn_degree: n=%d P=%d (n 2 .. %d, P = min(%d, n - 1))", n, P, KNN_MAX_ROWS, KNN_P_MAX);
  SDK_REQUIRE(p >= 1 && p <= P, "sdk_knn_degree: p=%d (1 .. P=%d)", p, P);
  SDK_REQUIRE(rev_off && rev_rank && deg && dinv, "sdk_knn_degree: null argument (rev_off=%p rev_rank=%p deg=%p dinv=%p)", (const void*)rev_off,
              (const void*)rev_rank, (void*)deg, (void*)dinv);
  hipLaunchKernelGGL(knn_degree_kernel, dim3((n + 3) / 4), dim3(KNN_NT), 0, (hipStream_t)stream, rev_off, rev_rank, n, p, deg, dinv);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_knn_matvec(sdk_ctx* ctx, const int32_t* idx, const int32_t* rev_off, const int32_t* rev_src, const int32_t* rev_rank,
                              const double* dinv, int n, int P, int p, const float* X, int kv, float* Y, void* stream) {
  SDK_REQUIRE(ctx, "sdk_knn_matvec: null context");
  SDK_REQUIRE(knn_shape_ok(n, P), "sdk_knn_matvec: n=%d P=%d (n 2 .. %d, P = min(%d, n - 1))", n, P, KNN_MAX_ROWS, KNN_P_MAX);
  SDK_REQUIRE(p >= 1 && p <= P, "sdk_knn_matvec: p=%d (1 .. P=%d)", p, P);
  SDK_REQUIRE(kv >= 1 && kv <= KNN_MAX_KV, "sdk_knn_matvec: kv=%d (1 .. %d)", kv, KNN_MAX_KV);
  SDK_REQUIRE(idx && rev_off && rev_src && rev_rank && dinv && X && Y && (const void*)X != (const void*)Y,
              "sdk_knn_matvec: null argument or X == Y (idx=%p rev_off=%p rev_src=%p rev_rank=%p dinv=%p X=%p Y=%p)", (const void*)idx,
              (const void*)rev_off, (const void*)rev_src, (const void*)rev_rank, (const void*)dinv, (const void*)X, (void*)Y);
  const int64_t m = (int64_t)n * kv;
  ProfScope ps(ctx, stream, SDK_K_COPY, 4.0 * (double)n * p * kv, (double)n * (8.0 * kv + 16.0 * p + 8.0));
  hipLaunchKernelGGL(knn_matvec_kernel, dim3((unsigned)((m + KNN_NT - 1) / KNN_NT)), dim3(KNN_NT), 0, (hipStream_t)stream, idx, rev_off, rev_src,
                     rev_rank, dinv, n, P, p, X, kv, Y);
  SDK_LAUNCH_CHECK();
  return 0;
}
