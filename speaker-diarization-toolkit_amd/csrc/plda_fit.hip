// Training the VBx PLDA from labelled embeddings (plda.fit): the sums over N labelled rows that the host's d x d solves start from, and the
// projection of every row into the LDA space.  Float64 results throughout.
//
//   pf_rowscale_kernel   wave = one fp32 row: s_i = sqrt(d) / max(|e_i - mean1|, 1e-300).  The stage-1 transform x1 = (e - mean1) s_i is then
//                        applied wherever the statistics kernels load a row, by the same two operations, so they all see the same bits
//                        (pf_project_kernel forms its own norm, in plda_front.hpp's order, and may differ from them in the last bit).
//   pf_count_kernel      counts [K] int64 by integer atomics (exact in any order); a label outside [0, K) is counted nowhere and sets status
//   pf_offsets_kernel    one block: the exclusive scan of the counts (the classes' segments of `order`)
//   pf_class_kernel      block = class, thread = the columns tid, tid + 256: the class's rows in the order of `order` (the stable sort of the
//                        row indices by label: ascending row index).  A row whose label is not the block's class is skipped and sets status.
//                        The walk over a class is serial, so the pass takes as long as the LARGEST class: meant for many classes of up to a
//                        few thousand rows (speakers), not for a few classes of 10^5 rows, which it serves correctly and slowly.
//   pf_colsum_kernel / pf_colsum_finish_kernel    the total: thread = column, one partial per row block, the partials in block order
//   pf_scatter_kernel    sum_i x_i x_i^T with v_mfma_f64_16x16x4_f64.  Grid (upper-triangle pairs of 64 x 64 macro tiles, row blocks); four
//                        waves, each a 32 x 32 quadrant = 2 x 2 MFMA tiles; rows enter 16 at a time through LDS (transformed once), the next
//                        16 are in flight in registers meanwhile.  A quadrant below the diagonal of a diagonal macro tile is not computed.
//   pf_scatter_finish_kernel   thread = an element (i <= j): the row blocks' partials in block order, written to [i][j] and [j][i]
//   pf_project_kernel    the front transform of plda_front.hpp, which plda_transform_kernel (vbx.hip) starts with too, for all rows, no row
//                        table: x2 = sqrt(D0) unit(lda^T x1 - mean2)
//
// Order of every sum (it depends on N, d, K and the labels only).  Rows are cut into nblk = ceil(N / RB) fixed blocks of
// RB = max(512, 64 ceil(N / 16384)) rows (at most 256 blocks).  An element of the scatter: inside a row block, four rows per MFMA in ascending
// order, accumulated in the instruction's C operand; then the blocks' partials in block order.  An element of the total: inside a row block
// ascending, then block order.  An element of a class sum: the class's rows in ascending row order.  No floating-point atomics, one owner per
// output element: two calls on the same input return the same bits.  Row offsets are 64-bit; N <= 2^24.
#include "common.hpp"
#include "plda_front.hpp"

#include <math.h>

namespace {

constexpr int PF_NT = 256;
constexpr int PF_MAX_ROWS = 1 << 24;
constexpr int PF_MT = 64;            // macro tile of the scatter
constexpr int PF_KC = 16;            // rows per LDS chunk
constexpr int PF_LD = 80;            // LDS row pitch in doubles: rows k and k + 1 of a fragment read fall into different halves of the banks
constexpr int PF_ST_LABEL = 1;

typedef double pf_d4 __attribute__((ext_vector_type(4)));

struct PfSrc {
  const float* E;                    // fp32 rows, or
  const double* X;                   // float64 rows as they lie
  const double* mean1;               // with E: centre and length-normalise (null: the rows as they are)
  const double* scale;               // s_i of pf_rowscale_kernel (with mean1)
  int d;
};

__device__ __forceinline__ double pf_at(const PfSrc& s, int64_t i, int j) {
  if (s.X) return s.X[i * s.d + j];
  const double e = (double)s.E[i * s.d + j];
  return s.mean1 ? (e - s.mean1[j]) * s.scale[i] : e;
}

__global__ __launch_bounds__(PF_NT) void pf_rowscale_kernel(const float* __restrict__ E, const double* __restrict__ mean1, int n, int d,
                                                            double* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (PF_NT / 64) + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* e = E + (int64_t)i * d;
  double q = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double v = (double)e[j] - mean1[j];
    q = fma(v, v, q);
  }
  q = wave_sum(q);
  if (lane == 0) scale[i] = sqrt((double)d) / fmax(sqrt(q), 1e-300);
}

__global__ __launch_bounds__(PF_NT) void pf_count_kernel(const int32_t* __restrict__ labels, int n, int K, int64_t* __restrict__ counts,
                                                         int32_t* __restrict__ status) {
  const int i = blockIdx.x * PF_NT + threadIdx.x;
  if (i >= n) return;
  const int lab = labels[i];
  if ((unsigned)lab < (unsigned)K) atomicAdd(reinterpret_cast<unsigned long long*>(counts + lab), 1ULL);
  else atomicOr(status, PF_ST_LABEL);
}

__global__ __launch_bounds__(1024) void pf_offsets_kernel(const int64_t* __restrict__ counts, int K, int64_t* __restrict__ off) {
  __shared__ int64_t s_part[1024];
  const int t = threadIdx.x, per = (K + 1023) / 1024;
  const int a = min(K, t * per), e = min(K, a + per);
  int64_t s = 0;
  for (int k = a; k < e; ++k) s += counts[k];
  s_part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int i = 0; i < 1024; ++i) {
      const int64_t v = s_part[i];
      s_part[i] = run;
      run += v;
    }
  }
  __syncthreads();
  int64_t run = s_part[t];
  for (int k = a; k < e; ++k) {
    off[k] = run;
    run += counts[k];
  }
  if (t == 1023) off[K] = run;
}

__global__ __launch_bounds__(PF_NT) void pf_class_kernel(PfSrc src, int n, const int32_t* __restrict__ labels, const int32_t* __restrict__ order,
                                                         const int64_t* __restrict__ off, double* __restrict__ sums, int32_t* __restrict__ status) {
  const int k = blockIdx.x, tid = threadIdx.x, d = src.d;
  const int j0 = tid, j1 = tid + PF_NT;
  const bool h0 = j0 < d, h1 = j1 < d;
  const int64_t p0 = off[k], p1 = off[k + 1];
  double a0 = 0.0, a1 = 0.0;
  for (int64_t p = p0; p < p1; ++p) {                                    // p1 <= n: the counts hold valid labels only
    const int r = order[p];
    if ((unsigned)r >= (unsigned)n || labels[r] != k) {                  // uniform over the block; only after a label outside [0, K)
      if (tid == 0) atomicOr(status, PF_ST_LABEL);
      continue;
    }
    if (h0) a0 += pf_at(src, r, j0);
    if (h1) a1 += pf_at(src, r, j1);
  }
  if (h0) sums[(int64_t)k * d + j0] = a0;
  if (h1) sums[(int64_t)k * d + j1] = a1;
}

__global__ __launch_bounds__(PF_NT) void pf_colsum_kernel(PfSrc src, int n, int RB, double* __restrict__ part) {
  const int b = blockIdx.x, d = src.d;
  const int i0 = b * RB, i1 = min(n, i0 + RB);
  for (int j = threadIdx.x; j < d; j += PF_NT) {
    double a = 0.0;
#pragma unroll 8
    for (int i = i0; i < i1; ++i) a += pf_at(src, i, j);
    part[(int64_t)b * d + j] = a;
  }
}

__global__ __launch_bounds__(PF_NT) void pf_colsum_finish_kernel(const double* __restrict__ part, int nblk, int d, double* __restrict__ total) {
  const int j = blockIdx.x * PF_NT + threadIdx.x;
  if (j >= d) return;
  double a = 0.0;
  for (int b = 0; b < nblk; ++b) a += part[(int64_t)b * d + j];
  total[j] = a;
}

__global__ __launch_bounds__(PF_NT) void pf_scatter_kernel(PfSrc src, int n, int RB, int nt, double* __restrict__ part) {
  __shared__ double s_a[PF_KC][PF_LD];
  __shared__ double s_b[PF_KC][PF_LD];
  const int tid = threadIdx.x, lane = tid & 63, d = src.d;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // blockIdx.x -> the macro tile (bi <= bj), row-major over the upper triangle
  int bi = 0, rest = blockIdx.x;
  while (rest >= nt - bi) { rest -= nt - bi; ++bi; }
  const int bj = bi + rest;
  const int qi = wave >> 1, qj = wave & 1;
  const bool active = !(bi == bj && qi > qj);                             // wave-uniform
  const int b = blockIdx.y;
  const int i0 = b * RB, i1 = min(n, i0 + RB);
  const int lr = tid >> 6, lc = tid & 63;                                 // a thread's elements of a panel: rows lr + 4 q, column lc
  const int ca = bi * PF_MT + lc, cb = bj * PF_MT + lc;
  double ra[4], rb[4];
  auto fetch = [&](int r0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = r0 + lr + 4 * q;
      const bool ok = i < i1;
      ra[q] = ok && ca < d ? pf_at(src, i, ca) : 0.0;
      rb[q] = ok && cb < d ? pf_at(src, i, cb) : 0.0;
    }
  };
  pf_d4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = pf_d4{0.0, 0.0, 0.0, 0.0};
  const int fk = lane >> 4, fc = lane & 15;
  fetch(i0);
  for (int r0 = i0; r0 < i1; r0 += PF_KC) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s_a[lr + 4 * q][lc] = ra[q];
      s_b[lr + 4 * q][lc] = rb[q];
    }
    __syncthreads();
    if (r0 + PF_KC < i1) fetch(r0 + PF_KC);                               // in flight during the MFMAs
    if (active) {
#pragma unroll
      for (int ks = 0; ks < PF_KC / 4; ++ks) {
        const int k = ks * 4 + fk;
        const double a0 = s_a[k][qi * 32 + fc], a1 = s_a[k][qi * 32 + 16 + fc];
        const double b0 = s_b[k][qj * 32 + fc], b1 = s_b[k][qj * 32 + 16 + fc];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
  double* P = part + (int64_t)b * d * d;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = bi * PF_MT + qi * 32 + u * 16 + fk + 4 * r;
        const int col = bj * PF_MT + qj * 32 + v * 16 + fc;
        if (row < d && col < d) P[(int64_t)row * d + col] = acc[u][v][r];
      }
}

__global__ __launch_bounds__(PF_NT) void pf_scatter_finish_kernel(const double* __restrict__ part, int nblk, int d, double* __restrict__ S) {
  const int e = blockIdx.x * PF_NT + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e % d;
  if (i > j) return;                                                      // (i, j) with i <= j lies in a computed quadrant
  const int64_t dd = (int64_t)d * d;
  double a = 0.0;
  for (int b = 0; b < nblk; ++b) a += part[b * dd + e];
  S[(int64_t)i * d + j] = a;
  S[(int64_t)j * d + i] = a;
}

__global__ __launch_bounds__(PLDA_NT) void pf_project_kernel(const float* __restrict__ E, int d_in, int n, const double* __restrict__ mean1,
                                                             const double* __restrict__ lda, const double* __restrict__ mean2, int D0,
                                                             double* __restrict__ X2) {
  __shared__ double s_a[PLDA_RPB][PLDA_MAX_DIM];
  __shared__ double s_red[PLDA_NT / 64];
  const int64_t i0 = (int64_t)blockIdx.x * PLDA_RPB;
  plda_front([&](int r) { return i0 + r < n ? E + (i0 + r) * d_in : nullptr; }, d_in, mean1, lda, mean2, D0, s_a, s_red,
             [&](int r, int j, double x2) { if (i0 + r < n) X2[(i0 + r) * D0 + j] = x2; });
}

inline int pf_row_block(int n) { return max(512, 64 * ((n + 16383) / 16384)); }

struct PfWs {
  double *scale, *colpart, *scatpart;
  int64_t* off;
};

size_t pf_carve(WsCarver c, int n, int d, int K, int with_scatter, PfWs* w) {
  const size_t nblk = (size_t)(n + pf_row_block(n) - 1) / pf_row_block(n);
  w->scale = c.take<double>((size_t)n);
  w->colpart = c.take<double>(nblk * d);
  w->scatpart = c.take<double>(with_scatter ? nblk * d * d : 0);
  w->off = c.take<int64_t>((size_t)K + 1);
  return c.bytes();
}

bool pf_shape_ok(int n, int d, int K) { return n >= 1 && n <= PF_MAX_ROWS && d >= 1 && d <= PLDA_MAX_DIM && K >= 0 && K <= PF_MAX_ROWS; }

}  // namespace

extern "C" size_t sdk_plda_fit_stats_workspace_bytes(int n, int d, int K, int with_scatter) {
  if (!pf_shape_ok(n, d, K)) {
    sdk_set_error("sdk_plda_fit_stats_workspace_bytes: n=%d d=%d K=%d (n 1 .. %d, d 1 .. %d, K 0 .. %d)", n, d, K, PF_MAX_ROWS, PLDA_MAX_DIM, PF_MAX_ROWS);
    return 0;
  }
  PfWs w;
  return pf_carve({}, n, d, K, with_scatter, &w);
}

extern "C" int sdk_plda_fit_stats(sdk_ctx* ctx, const float* E, const double* X, const double* mean1, int n, int d, const int32_t* labels,
                                  const int32_t* order, int K, int64_t* counts, double* sums, double* total, double* scatter, int32_t* status,
                                  void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx, "sdk_plda_fit_stats: null context");
  SDK_REQUIRE(n >= 1 && n <= PF_MAX_ROWS, "sdk_plda_fit_stats: n=%d rows (1 .. %d)", n, PF_MAX_ROWS);
  SDK_REQUIRE((E != nullptr) != (X != nullptr), "sdk_plda_fit_stats: exactly one source (E=%p fp32 rows, X=%p float64 rows)", (const void*)E,
              (const void*)X);
  if (E) SDK_REQUIRE(d >= 64 && d <= PLDA_MAX_DIM && d % 64 == 0, "sdk_plda_fit_stats: d=%d not supported for fp32 rows (a multiple of 64, at most %d)", d, PLDA_MAX_DIM);
  else SDK_REQUIRE(d >= 1 && d <= PLDA_MAX_DIM && !mean1, "sdk_plda_fit_stats: float64 rows take d=%d in 1 .. %d and no mean1", d, PLDA_MAX_DIM);
  SDK_REQUIRE(K >= 0 && K <= PF_MAX_ROWS, "sdk_plda_fit_stats: K=%d classes (0 .. %d)", K, PF_MAX_ROWS);
  if (K > 0) SDK_REQUIRE(labels && order && counts && sums, "sdk_plda_fit_stats: K=%d needs labels=%p order=%p counts=%p sums=%p", K,
                         (const void*)labels, (const void*)order, (void*)counts, (void*)sums);
  SDK_REQUIRE(total && status && ws, "sdk_plda_fit_stats: null argument (total=%p status=%p ws=%p)", (void*)total, (void*)status, ws);
  SDK_REQUIRE_WS("sdk_plda_fit_stats", "sdk_plda_fit_stats_workspace_bytes", ws, ws_bytes,
                 sdk_plda_fit_stats_workspace_bytes(n, d, K, scatter != nullptr), 256);
  PfWs w;
  pf_carve({static_cast<char*>(ws), 0}, n, d, K, scatter != nullptr, &w);
  hipStream_t st = (hipStream_t)stream;
  const int RB = pf_row_block(n), nblk = (n + RB - 1) / RB;
  const PfSrc src{E, X, mean1, w.scale, d};
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)n * d * (E ? 4.0 : 8.0) * (scatter ? 3.0 : 2.0));      // booked as bytes moved; no flop count under this kind
  SDK_HIP_OK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (E && mean1) hipLaunchKernelGGL(pf_rowscale_kernel, dim3((n + 3) / 4), dim3(PF_NT), 0, st, E, mean1, n, d, w.scale);
  if (K > 0) {
    SDK_HIP_OK(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int64_t), st));
    hipLaunchKernelGGL(pf_count_kernel, dim3((n + PF_NT - 1) / PF_NT), dim3(PF_NT), 0, st, labels, n, K, counts, status);
    hipLaunchKernelGGL(pf_offsets_kernel, dim3(1), dim3(1024), 0, st, counts, K, w.off);
    hipLaunchKernelGGL(pf_class_kernel, dim3(K), dim3(PF_NT), 0, st, src, n, labels, order, w.off, sums, status);
  }
  hipLaunchKernelGGL(pf_colsum_kernel, dim3(nblk), dim3(PF_NT), 0, st, src, n, RB, w.colpart);
  hipLaunchKernelGGL(pf_colsum_finish_kernel, dim3((d + PF_NT - 1) / PF_NT), dim3(PF_NT), 0, st, w.colpart, nblk, d, total);
  if (scatter) {
    const int nt = (d + PF_MT - 1) / PF_MT;
    hipLaunchKernelGGL(pf_scatter_kernel, dim3(nt * (nt + 1) / 2, nblk), dim3(PF_NT), 0, st, src, n, RB, nt, w.scatpart);
    hipLaunchKernelGGL(pf_scatter_finish_kernel, dim3((d * d + PF_NT - 1) / PF_NT), dim3(PF_NT), 0, st, w.scatpart, nblk, d, scatter);
  }
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_plda_project(sdk_ctx* ctx, const float* E, int d_in, int n, const double* mean1, const double* lda, const double* mean2, int D0,
                                double* X2, void* stream) {
  SDK_REQUIRE(ctx, "sdk_plda_project: null context");
  SDK_REQUIRE(n >= 1 && n <= PF_MAX_ROWS, "sdk_plda_project: n=%d rows (1 .. %d)", n, PF_MAX_ROWS);
  SDK_REQUIRE(d_in >= 64 && d_in <= PLDA_MAX_DIM && d_in % 64 == 0, "sdk_plda_project: d_in=%d not supported (a multiple of 64, at most %d)", d_in,
              PLDA_MAX_DIM);
  SDK_REQUIRE(D0 >= 1 && D0 <= PLDA_MAX_DIM, "sdk_plda_project: D0=%d (1 .. %d)", D0, PLDA_MAX_DIM);
  SDK_REQUIRE(E && mean1 && lda && mean2 && X2, "sdk_plda_project: null argument (E=%p mean1=%p lda=%p mean2=%p X2=%p)", (const void*)E,
              (const void*)mean1, (const void*)lda, (const void*)mean2, (void*)X2);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)n * (4.0 * d_in + 8.0 * D0) + 8.0 * D0 * d_in);
  hipLaunchKernelGGL(pf_project_kernel, dim3((n + PLDA_RPB - 1) / PLDA_RPB), dim3(PLDA_NT), 0, (hipStream_t)stream, E, d_in, n, mean1, lda, mean2, D0, X2);
  SDK_LAUNCH_CHECK();
  return 0;
}
