// The packed frame grid shared by the grouped kernels (diarize.hip, score.hip, score_jer.hip, words.hip, samples.hip, smooth.hip): R recordings
// laid end to end on one axis - frames, words, clusters, reference speakers or co cells - with a prefix-sum table off [R + 1] per axis
// (frame_off, word_off, cent_off, ref_off, co_off).  Each of these is written here once:
//
//   PG_HOP, PG_FIRST   frame g of a recording has centre sample PG_HOP g + PG_FIRST (diarize.global_frames); pg_first_frame is the grid's
//                      one rounding rule.
//   pg_find_group      an element's recording, by binary search on the table that counts such elements (no per-element table is built).
//   PG_MAX_SPK         the speakers a side of a scoring table; pg_speakers reads a recording's count clamped to it.
//   pg_grid            the launch grid of `n` elements taken `per` workgroup.
//   pg_walk            a workgroup takes a span [x0, x1) of a packed axis and serves the recordings inside it one at a time
//                      (score_cooccur_kernel, score_durations_kernel, words_cooccur_kernel).
//   pg_co_clear,       the LDS co table [S_r][K_r] and the N tallies of the two co-occurrence kernels around their counting loops: cleared
//   pg_co_flush        before, then one integer global atomic per non-zero cell and tally.  Integer adds do not depend on the order they land
//                      in, so the tables are bit-identical run to run.
#pragma once

#include "common.hpp"

namespace {

constexpr int PG_HOP = 270, PG_FIRST = 495;  // segmentation.FRAME_HOP, segmentation.FRAME_FIRST
constexpr int PG_MAX_SPK = 64;               // reference and hypothesis speakers per recording in a scoring table (score.MAX_SCORE_SPEAKERS)

// the least g >= 0 with PG_HOP g + PG_FIRST >= s (int64: s + PG_HOP - 1 may pass 2^31).  The frames lo <= g < hi with lo = pg_first_frame(s0),
// hi = pg_first_frame(s1) are those with s0 <= centre < s1, and pg_first_frame(n_samples) is the number of frames of a recording
__host__ __device__ __forceinline__ int64_t pg_first_frame(int64_t s) {
  const int64_t a = s - PG_FIRST;
  return a <= 0 ? 0 : (a + PG_HOP - 1) / PG_HOP;
}

// the r with off[r] <= x < off[r + 1], for 0 <= x < off[R] (groups without elements are stepped over).  T: int32_t, or int64_t for co_off
template <class T>
__device__ __forceinline__ int pg_find_group(const T* __restrict__ off, int R, T x) {
  int lo = 0, hi = R;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// the group of x for a thread that steps through ascending x, from the group r of an earlier x: never past R - 1, whatever x is
__device__ __forceinline__ int pg_next_group(const int32_t* __restrict__ off, int R, int r, int x) {
  while (r + 1 < R && off[r + 1] <= x) ++r;
  return r;
}

// the speakers recording r has on the side that off counts (ref_off or cent_off), clamped to 0 .. PG_MAX_SPK whatever the table says
__device__ __forceinline__ int pg_speakers(const int32_t* __restrict__ off, int r) { return min(max(off[r + 1] - off[r], 0), PG_MAX_SPK); }

static inline dim3 pg_grid(int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

// Calls body(r, a, b) once per recording r that has elements in [x0, x1), in ascending order: [a, b) is the part of [x0, x1) that lies in
// recording r.  x0 and x1 must be uniform over the workgroup and x1 <= off[R]; then every argument of the body and every quantity of the
// loop is uniform too: the body may hold barriers; the walk never diverges.  A body that reuses LDS ends with a barrier of its own.
template <class Body>
__device__ __forceinline__ void pg_walk(const int32_t* __restrict__ off, int R, int x0, int x1, Body body) {
  if (x0 >= x1) return;
  int r = pg_find_group(off, R, x0);
  for (int a = x0; a < x1;) {
    while (off[r + 1] <= a) ++r;                                // a < x1 <= off[R]: ends with r < R
    const int b = min(x1, off[r + 1]);
    body(r, a, b);
    a = b;
  }
}

// before a recording's counting loop: `cells` entries of the LDS table and the N tallies = 0, then a barrier.  NT: threads of the workgroup
template <int N, int NT>
__device__ __forceinline__ void pg_co_clear(int32_t* tab, int32_t* tal, int cells) {
  const int tid = threadIdx.x;
  for (int c = tid; c < cells; c += NT) tab[c] = 0;
  if (tid < N) tal[tid] = 0;
  __syncthreads();
}

// after it: the thread's N counts n are summed over the wave and the workgroup into tal; then one global atomic add per non-zero cell to
// dst [cells] and per non-zero tally to tally [N] (unsigned 64-bit), and the barrier after which the table may be cleared again
template <int N, int NT>
__device__ __forceinline__ void pg_co_flush(const int32_t* tab, int32_t* tal, const int (&n)[N], int cells, int32_t* __restrict__ dst,
                                            unsigned long long* __restrict__ tally) {
  const int tid = threadIdx.x;
  int s[N];
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = wave_sum(n[k]);            // the N shuffle chains first, so that they overlap
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) atomicAdd(&tal[k], s[k]);
  }
  __syncthreads();
  for (int c = tid; c < cells; c += NT) {
    const int v = tab[c];
    if (v) atomicAdd(dst + c, v);
  }
  if (tid < N && tal[tid]) atomicAdd(tally + tid, (unsigned long long)tal[tid]);
  __syncthreads();
}

}  // namespace
