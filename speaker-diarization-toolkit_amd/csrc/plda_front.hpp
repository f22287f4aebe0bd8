// The PLDA front transform, shared by plda_transform_kernel (vbx.hip) and pf_project_kernel (plda_fit.hip):
//   x1 = sqrt(d_in) unit(e - mean1),   x2 = sqrt(D0) unit(lda^T x1 - mean2)      float64
// One body, so the two entry points return the same bits for the same row (tests/test_plda_fit_gpu.py::test_projection asserts it).
#pragma once
#include "common.hpp"

#include <math.h>

constexpr int PLDA_NT = 256;         // threads of the block: thread = the columns tid and tid + 256
constexpr int PLDA_RPB = 4;          // rows per block
constexpr int PLDA_MAX_DIM = 512;    // d_in and D0: two columns per thread

// For the block's PLDA_RPB rows: row(r) returns row r's fp32 embedding, or nullptr for a row past the end (the same answer in every thread:
// a short last block runs every barrier, on zeros); store(r, j, x2[r][j]) is called by the thread that owns column j < D0, for every r.
// s_a is the stage-1 scratch, s_red the scratch of block_sum.  Every dot product runs over its index in ascending order, as one fma chain.
// Nothing of `store` is visible to the block's other threads before the caller's next barrier.
template <class Row, class Store>
__device__ __forceinline__ void plda_front(Row row, int d_in, const double* __restrict__ mean1, const double* __restrict__ lda,
                                           const double* __restrict__ mean2, int D0, double (*s_a)[PLDA_MAX_DIM], double* s_red, Store store) {
  const int j0 = threadIdx.x, j1 = threadIdx.x + PLDA_NT;
  // 1: x1 = sqrt(d_in) unit(e - mean1)
  for (int r = 0; r < PLDA_RPB; ++r) {
    const float* e = row(r);                                             // uniform over the block
    const double v0 = e && j0 < d_in ? (double)e[j0] - mean1[j0] : 0.0;
    const double v1 = e && j1 < d_in ? (double)e[j1] - mean1[j1] : 0.0;
    const double nrm = block_sum(fma(v0, v0, v1 * v1), s_red);
    const double sc = sqrt((double)d_in) / fmax(sqrt(nrm), 1e-300);
    if (j0 < d_in) s_a[r][j0] = v0 * sc;
    if (j1 < d_in) s_a[r][j1] = v1 * sc;
  }
  __syncthreads();
  // 2: x2 = sqrt(D0) unit(lda^T x1 - mean2)
  double a0[PLDA_RPB], a1[PLDA_RPB];
#pragma unroll
  for (int r = 0; r < PLDA_RPB; ++r) a0[r] = a1[r] = 0.0;
  for (int i = 0; i < d_in; ++i) {
    const double l0 = j0 < D0 ? lda[(int64_t)i * D0 + j0] : 0.0;
    const double l1 = j1 < D0 ? lda[(int64_t)i * D0 + j1] : 0.0;
#pragma unroll
    for (int r = 0; r < PLDA_RPB; ++r) {
      const double x = s_a[r][i];
      a0[r] = fma(x, l0, a0[r]);
      a1[r] = fma(x, l1, a1[r]);
    }
  }
  for (int r = 0; r < PLDA_RPB; ++r) {
    const double v0 = j0 < D0 ? a0[r] - mean2[j0] : 0.0;
    const double v1 = j1 < D0 ? a1[r] - mean2[j1] : 0.0;
    const double nrm = block_sum(fma(v0, v0, v1 * v1), s_red);
    const double sc = sqrt((double)D0) / fmax(sqrt(nrm), 1e-300);
    if (j0 < D0) store(r, j0, v0 * sc);
    if (j1 < D0) store(r, j1, v1 * sc);
  }
}
