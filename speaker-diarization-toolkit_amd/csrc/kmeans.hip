// Spherical k-means on unit rows (cluster.kmeans_cluster): the forced speaker count of the diarization, `speakers=`, with clustering="vbx".
// The thin k-means of spectral.hip serves rows of at most 32 fp32 columns; this one serves the embedding widths of sdk_diarize_assign
// (d = 64, 128, .. 512), up to 64 centres and 65 536 rows, in float64, and enqueues the whole Lloyd loop at once.
//
//   km_reset_kernel       n_iter = status = done = changed = 0
//   km_init_kernel        wave = one row: a non-finite value sets status and done; labels = -1
//   km_seed_pick_kernel   centre j = row 0 (j = 0), else the row of least maxcos (ties to the lowest row) from the blocks' candidates
//   km_seed_dist_kernel   thread = one row: its cosine to centre j, ONE fma chain over the columns in ascending order (a seed is a row, so
//                         every product is exact and the chain equals the plain sum); maxcos = max(maxcos, cos); the block's least
//   km_assign_kernel      workgroup = 32 rows, wave = 8 of them, lane = one centre.  The centres, kept transposed (Ct [d][64] float64), pass
//                         through LDS in tiles of 64 columns beside the rows' columns as float64; a lane runs one fma chain per row over
//                         the columns in ascending order.  The arg-max over the centres is a wave reduction on (cosine, centre): the larger
//                         cosine, then the lower centre; a NaN, or a lane past k, holds no candidate.
//   km_step_kernel        n_iter = it + 1; from it = 1 on, an assignment that changed no label sets done
//   km_sums_kernel        workgroup = (1024-row segment, centre): the segment's rows with that label, listed in ascending order by one wave
//                         (ballot + popcount), summed in that order in float64, thread = columns tid, tid + 256
//   km_finish_kernel      workgroup = centre: the segments' partials in segment order, the norm (block_sum, reduce.hpp), c = s / |s|; a centre without
//                         rows, or with |s| = 0, is left as it was
//
// Every launch after `done` leaves at its first instruction, as in vbx.hip.  No floating-point atomics, one owner per output element, every
// sum in one fixed order: bit-identical run to run.  No workgroup waits for another: an iteration is four launches on the caller's stream.
#include "common.hpp"

#include <climits>

namespace {

constexpr int KM_NT = 256;
constexpr int KM_MAX_K = 64;         // centres: one lane each (cluster.KMEANS_MAX_K)
constexpr int KM_MAX_D = 512;
constexpr int KM_MAX_ROWS = 65536;
constexpr int KM_RB = 32;            // rows per workgroup of the assignment
constexpr int KM_RW = KM_RB / 4;     // rows per wave
constexpr int KM_TJ = 64;            // columns per LDS tile
constexpr int KM_SEG = 1024;         // rows per segment of the centre sums (cluster.KMEANS_SEGMENT)
constexpr int KM_ST_NONFINITE = 1;

struct KmWs {
  double* Ct;        // [d][64] centres, transposed
  double* maxcos;    // [n]
  double* sval;      // [ceil(n / 256)] the seed blocks' least maxcos
  int32_t* srow;     // [ceil(n / 256)] and its row
  double* psum;      // [nseg][k][d]
  int32_t* pcnt;     // [nseg][k]
  int32_t* done;
  int32_t* changed;
};

size_t km_carve(WsCarver c, int n, int d, int k, KmWs* w) {
  const size_t nblk = (size_t)(n + KM_NT - 1) / KM_NT, nseg = (size_t)(n + KM_SEG - 1) / KM_SEG;
  w->Ct = c.take<double>((size_t)d * KM_MAX_K);
  w->maxcos = c.take<double>(n);
  w->sval = c.take<double>(nblk);
  w->srow = c.take<int32_t>(nblk);
  w->psum = c.take<double>(nseg * k * d);
  w->pcnt = c.take<int32_t>(nseg * k);
  w->done = c.take<int32_t>(1);
  w->changed = c.take<int32_t>(1);
  return c.bytes();
}

bool km_shape_ok(int n, int d, int k) {
  return n >= 1 && n <= KM_MAX_ROWS && d >= 64 && d <= KM_MAX_D && d % 64 == 0 && k >= 1 && k <= KM_MAX_K && k <= n;
}

__global__ __launch_bounds__(64) void km_reset_kernel(int32_t* __restrict__ n_iter, int32_t* __restrict__ status, KmWs w) {
  if (threadIdx.x == 0) {
    *n_iter = 0;
    *status = 0;
    *w.done = 0;
    *w.changed = 0;
  }
}

__global__ __launch_bounds__(KM_NT) void km_init_kernel(const float* __restrict__ E, const int32_t* __restrict__ rows, int n, int d,
                                                        int32_t* __restrict__ labels, int32_t* __restrict__ status, KmWs w) {
  const int t = blockIdx.x * (KM_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= n) return;                                  // uniform over the wave
  const float* e = E + (int64_t)rows[t] * d;
  bool bad = false;
  for (int j = lane; j < d; j += 64) bad |= !isfinite(e[j]);
  const bool any_bad = __ballot(bad) != 0;
  if (lane == 0) {
    labels[t] = -1;
    if (any_bad) { atomicOr(status, KM_ST_NONFINITE); *w.done = 1; }
  }
}

// (value, row) with the smaller value first, ties to the lower row; row == INT_MAX: nothing
__device__ __forceinline__ bool km_less(double v, int r, double bv, int br) { return r != INT_MAX && (br == INT_MAX || v < bv || (v == bv && r < br)); }

__device__ __forceinline__ void km_block_argmin(double& v, int& r, double* s_v, int* s_r) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int orow = __shfl_xor(r, o, 64);
    if (km_less(ov, orow, v, r)) { v = ov; r = orow; }
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { s_v[tid >> 6] = v; s_r[tid >> 6] = r; }
  __syncthreads();
  v = s_v[0];
  r = s_r[0];
#pragma unroll
  for (int q = 1; q < KM_NT / 64; ++q)
    if (km_less(s_v[q], s_r[q], v, r)) { v = s_v[q]; r = s_r[q]; }
}

__global__ __launch_bounds__(KM_NT) void km_seed_pick_kernel(const float* __restrict__ E, const int32_t* __restrict__ rows, int d, int j, int nblk,
                                                             KmWs w) {
  __shared__ double s_v[KM_NT / 64];
  __shared__ int s_r[KM_NT / 64];
  if (*w.done) return;
  const int tid = threadIdx.x;
  int pick = 0;
  if (j > 0) {
    double v = 0.0;
    int r = INT_MAX;
    if (tid < nblk) { v = w.sval[tid]; r = w.srow[tid]; }        // nblk <= 256: n <= 65 536
    km_block_argmin(v, r, s_v, s_r);
    pick = r == INT_MAX ? 0 : r;
  }
  const float* e = E + (int64_t)rows[pick] * d;
  for (int c = tid; c < d; c += KM_NT) w.Ct[(int64_t)c * KM_MAX_K + j] = (double)e[c];
}

__global__ __launch_bounds__(KM_NT) void km_seed_dist_kernel(const float* __restrict__ E, const int32_t* __restrict__ rows, int n, int d, int j,
                                                             KmWs w) {
  __shared__ float s_x[KM_NT][33];
  __shared__ double s_v[KM_NT / 64];
  __shared__ int s_r[KM_NT / 64];
  if (*w.done) return;
  const int tid = threadIdx.x, t0 = blockIdx.x * KM_NT, t = t0 + tid;
  const int m = min(KM_NT, n - t0);
  const double* cj = w.Ct + j;
  double acc = 0.0;
  for (int c0 = 0; c0 < d; c0 += 32) {
    __syncthreads();
    for (int p = 0; p < 32; ++p) {                     // 8 rows of 32 columns (128 bytes each) per pass
      const int r = (tid >> 5) + 8 * p;
      s_x[r][tid & 31] = r < m ? E[(int64_t)rows[t0 + r] * d + c0 + (tid & 31)] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int jj = 0; jj < 32; ++jj) acc = fma((double)s_x[tid][jj], cj[(int64_t)(c0 + jj) * KM_MAX_K], acc);
  }
  double v = 0.0;
  int r = INT_MAX;
  if (t < n) {
    v = j == 0 ? acc : fmax(w.maxcos[t], acc);
    w.maxcos[t] = v;
    r = t;
  }
  km_block_argmin(v, r, s_v, s_r);
  if (tid == 0) { w.sval[blockIdx.x] = v; w.srow[blockIdx.x] = r; }
}

// (value, centre) with the larger value first, ties to the lower centre; centre < 0: nothing
__device__ __forceinline__ bool km_better(double v, int k, double bv, int bk) { return k >= 0 && (bk < 0 || v > bv || (v == bv && k < bk)); }

__global__ __launch_bounds__(KM_NT) void km_assign_kernel(const float* __restrict__ E, const int32_t* __restrict__ rows, int n, int d, int k,
                                                          int32_t* __restrict__ labels, KmWs w) {
  __shared__ double s_c[KM_TJ][KM_MAX_K];              // 32 KB: a tile of the transposed centres
  __shared__ double s_e[KM_RB][KM_TJ];                 // 16 KB: the same columns of the workgroup's rows
  if (*w.done) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, t0 = blockIdx.x * KM_RB;
  double acc[KM_RW];
#pragma unroll
  for (int q = 0; q < KM_RW; ++q) acc[q] = 0.0;
  for (int c0 = 0; c0 < d; c0 += KM_TJ) {
    __syncthreads();
    const double* src = w.Ct + (int64_t)c0 * KM_MAX_K;
    for (int i = tid; i < KM_TJ * KM_MAX_K; i += KM_NT) (&s_c[0][0])[i] = src[i];
    for (int i = tid; i < KM_RB * KM_TJ; i += KM_NT) {
      const int r = i / KM_TJ, c = i - r * KM_TJ, t = t0 + r;
      s_e[r][c] = t < n ? (double)E[(int64_t)rows[t] * d + c0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < KM_TJ; ++jj) {
      const double c = s_c[jj][lane];
#pragma unroll
      for (int q = 0; q < KM_RW; ++q) acc[q] = fma(s_e[wave * KM_RW + q][jj], c, acc[q]);
    }
  }
  bool ch = false;
#pragma unroll
  for (int q = 0; q < KM_RW; ++q) {
    const int t = t0 + wave * KM_RW + q;
    if (t >= n) break;                                 // uniform over the wave
    double v = acc[q];
    int kk = (lane < k && v == v) ? lane : -1;         // a NaN never wins
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int ok = __shfl_xor(kk, o, 64);
      if (km_better(ov, ok, v, kk)) { v = ov; kk = ok; }
    }
    if (lane == 0) {
      if (labels[t] != kk) ch = true;
      labels[t] = kk;
    }
  }
  if (ch) *w.changed = 1;
}

__global__ __launch_bounds__(64) void km_step_kernel(int it, int32_t* __restrict__ n_iter, KmWs w) {
  if (threadIdx.x != 0 || *w.done) return;
  *n_iter = it + 1;
  if (it >= 1 && *w.changed == 0) *w.done = 1;
  *w.changed = 0;
}

__global__ __launch_bounds__(KM_NT) void km_sums_kernel(const float* __restrict__ E, const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ labels, int n, int d, int k, KmWs w) {
  __shared__ int32_t s_list[KM_SEG];
  __shared__ int s_cnt;
  if (*w.done) return;
  const int seg = blockIdx.x, kk = blockIdx.y, tid = threadIdx.x;
  const int t0 = seg * KM_SEG, m = min(KM_SEG, n - t0);
  if (tid < 64) {                                      // wave 0 lists the segment's rows labelled kk, in ascending order
    int base = 0;
    for (int i0 = 0; i0 < m; i0 += 64) {
      const int i = i0 + tid;
      const bool hit = i < m && labels[t0 + i] == kk;
      const unsigned long long mask = __ballot(hit);
      if (hit) s_list[base + __popcll(mask & ((1ull << tid) - 1ull))] = rows[t0 + i];
      base += __popcll(mask);
    }
    if (tid == 0) s_cnt = base;
  }
  __syncthreads();
  const int cnt = s_cnt, j0 = tid, j1 = tid + KM_NT;
  double a0 = 0.0, a1 = 0.0;
#pragma unroll 4
  for (int i = 0; i < cnt; ++i) {
    const float* e = E + (int64_t)s_list[i] * d;
    if (j0 < d) a0 += (double)e[j0];
    if (j1 < d) a1 += (double)e[j1];
  }
  double* out = w.psum + ((int64_t)seg * k + kk) * d;
  if (j0 < d) out[j0] = a0;
  if (j1 < d) out[j1] = a1;
  if (tid == 0) w.pcnt[seg * k + kk] = cnt;
}

__global__ __launch_bounds__(KM_NT) void km_finish_kernel(int nseg, int d, int k, KmWs w) {
  __shared__ double s_red[KM_NT / 64];
  if (*w.done) return;
  const int kk = blockIdx.x, tid = threadIdx.x, j0 = tid, j1 = tid + KM_NT;
  double a0 = 0.0, a1 = 0.0;
  int cnt = 0;
  for (int s = 0; s < nseg; ++s) {
    const double* p = w.psum + ((int64_t)s * k + kk) * d;
    if (j0 < d) a0 += p[j0];
    if (j1 < d) a1 += p[j1];
    cnt += w.pcnt[s * k + kk];
  }
  const double nrm = sqrt(block_sum((j0 < d ? a0 * a0 : 0.0) + (j1 < d ? a1 * a1 : 0.0), s_red));
  if (cnt == 0 || !(nrm > 0.0)) return;                // uniform over the workgroup: the centre stays
  if (j0 < d) w.Ct[(int64_t)j0 * KM_MAX_K + kk] = a0 / nrm;
  if (j1 < d) w.Ct[(int64_t)j1 * KM_MAX_K + kk] = a1 / nrm;
}

}  // namespace

extern "C" size_t sdk_kmeans_rows_workspace_bytes(int n, int d, int k) {
  if (!km_shape_ok(n, d, k)) {
    sdk_set_error("sdk_kmeans_rows_workspace_bytes: n=%d d=%d k=%d (n 1 .. %d, d a multiple of 64 up to %d, k 1 .. min(n, %d))", n, d, k, KM_MAX_ROWS,
                  KM_MAX_D, KM_MAX_K);
    return 0;
  }
  KmWs w;
  return km_carve({}, n, d, k, &w);
}

extern "C" int sdk_kmeans_rows(sdk_ctx* ctx, const float* E, const int32_t* rows, int n, int d, int k, int max_iters, int32_t* labels,
                               int32_t* n_iter, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx, "sdk_kmeans_rows: null context");
  SDK_REQUIRE(n >= 1 && n <= KM_MAX_ROWS, "sdk_kmeans_rows: n=%d (1 .. %d)", n, KM_MAX_ROWS);
  SDK_REQUIRE(d >= 64 && d <= KM_MAX_D && d % 64 == 0, "sdk_kmeans_rows: d=%d not supported (a multiple of 64, at most %d)", d, KM_MAX_D);
  SDK_REQUIRE(k >= 1 && k <= KM_MAX_K && k <= n, "sdk_kmeans_rows: k=%d (1 .. min(n, %d), n=%d)", k, KM_MAX_K, n);
  SDK_REQUIRE(max_iters >= 1 && max_iters <= 1000, "sdk_kmeans_rows: max_iters=%d (1 .. 1000)", max_iters);
  SDK_REQUIRE(E && rows && labels && n_iter && status && ws, "sdk_kmeans_rows: null argument (E=%p rows=%p labels=%p n_iter=%p status=%p ws=%p)",
              (const void*)E, (const void*)rows, (void*)labels, (void*)n_iter, (void*)status, ws);
  SDK_REQUIRE_WS("sdk_kmeans_rows", "sdk_kmeans_rows_workspace_bytes", ws, ws_bytes, sdk_kmeans_rows_workspace_bytes(n, d, k), 256);
  KmWs w;
  km_carve({static_cast<char*>(ws), 0}, n, d, k, &w);
  const int nblk = (n + KM_NT - 1) / KM_NT, nseg = (n + KM_SEG - 1) / KM_SEG;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * max_iters * (double)n * k * d, (double)max_iters * n * (8.0 * d + 8.0));
  hipLaunchKernelGGL(km_reset_kernel, dim3(1), dim3(64), 0, st, n_iter, status, w);
  hipLaunchKernelGGL(km_init_kernel, dim3((n + 3) / 4), dim3(KM_NT), 0, st, E, rows, n, d, labels, status, w);
  hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), dim3(KM_NT), 0, st, E, rows, d, 0, nblk, w);
  for (int j = 1; j < k; ++j) {
    hipLaunchKernelGGL(km_seed_dist_kernel, dim3(nblk), dim3(KM_NT), 0, st, E, rows, n, d, j - 1, w);
    hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), dim3(KM_NT), 0, st, E, rows, d, j, nblk, w);
  }
  for (int it = 0; it < max_iters; ++it) {
    hipLaunchKernelGGL(km_assign_kernel, dim3((n + KM_RB - 1) / KM_RB), dim3(KM_NT), 0, st, E, rows, n, d, k, labels, w);
    hipLaunchKernelGGL(km_step_kernel, dim3(1), dim3(64), 0, st, it, n_iter, w);
    if (it + 1 == max_iters) break;                    // the last assignment's labels are the result: no centre is read after it
    hipLaunchKernelGGL(km_sums_kernel, dim3(nseg, k), dim3(KM_NT), 0, st, E, rows, labels, n, d, k, w);
    hipLaunchKernelGGL(km_finish_kernel, dim3(k), dim3(KM_NT), 0, st, nseg, d, k, w);
  }
  SDK_LAUNCH_CHECK();
  return 0;
}
