// The pieces of the diarization kernels that csrc/diarize.hip and csrc/stream.hip share: the powerset's class masks, the frame grid, and the
// assignment of one chunk's candidates to unit centroids (diarize.py "assignment" and "constrained assignment").
#pragma once
#include "common.hpp"
#include "packed_grid.hpp"

namespace {

constexpr int DZ_HOP = PG_HOP;       // samples between segmentation frames: the chunk grid's name for the hop of the global frame grid
constexpr int DZ_MAX_D = 512;        // embedding width served by the assignment (a multiple of 64)

// the speakers of powerset class c = {}, {0}, {1}, {2}, {0,1}, {0,2}, {1,2} as a 3-bit mask (0 for anything else)
__device__ __forceinline__ int cls_mask(int c) { return (unsigned)c < 7u ? (0x6534210 >> (4 * c)) & 7 : 0; }

// q_c = floor((DZ_HOP / 2 - start_c) / DZ_HOP): global frame g reads frame g + q_c of chunk c
__device__ __forceinline__ int64_t chunk_q(int64_t start) {
  const int64_t a = DZ_HOP / 2 - start;
  return a >= 0 ? a / DZ_HOP : -((-a + DZ_HOP - 1) / DZ_HOP);
}

// global frames of a recording of n_samples samples (diarize.global_frames): the frames whose centre lies before its end
__host__ __device__ inline int64_t dz_frames(int64_t n_samples) { return pg_first_frame(n_samples); }

// (value, cluster) lists of a row's three largest cosines, best first; ties to the lower cluster; idx < 0: empty
struct Top3 { double v[3]; int k[3]; };

__device__ __forceinline__ bool better(double v, int k, double bv, int bk) { return bk < 0 || v > bv || (v == bv && k < bk); }

__device__ __forceinline__ void top3_push(Top3& t, double v, int k) {
  if (!(v == v)) return;                               // a NaN never wins
  if (better(v, k, t.v[0], t.k[0])) {
    t.v[2] = t.v[1]; t.k[2] = t.k[1]; t.v[1] = t.v[0]; t.k[1] = t.k[0]; t.v[0] = v; t.k[0] = k;
  } else if (better(v, k, t.v[1], t.k[1])) {
    t.v[2] = t.v[1]; t.k[2] = t.k[1]; t.v[1] = v; t.k[1] = k;
  } else if (better(v, k, t.v[2], t.k[2])) {
    t.v[2] = v; t.k[2] = k;
  }
}

// what a chunk's assignment keeps in LDS: its candidate rows as float64, and per candidate the three best (cosine, cluster) of the wave
struct AssignLds {
  double e[3][DZ_MAX_D];
  double v[3][3];
  int k[3][3];
};

// info [3][4] of a chunk -> its candidates: valid and with an active frame
__device__ __forceinline__ void assign_candidates(const int32_t* __restrict__ info, bool cand[3]) {
#pragma unroll
  for (int s = 0; s < 3; ++s) cand[s] = info[s * 4 + 3] != 0 && info[s * 4] > 0;
}

// the chunk's candidate rows (E: its three rows) go to LDS as float64, by the threads tid, tid + nt, ..; rows that are no candidates are
// never read.  A workgroup barrier belongs between this and assign_solve.
__device__ __forceinline__ void assign_stage(AssignLds& L, const float* __restrict__ E, const bool cand[3], int d, int tid, int nt) {
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (cand[s]) {
      const float* e = E + (int64_t)s * d;
      for (int j = tid; j < d; j += nt) L.e[s][j] = (double)e[j];
    }
  }
}

// ONE wave.  Lane l takes the clusters l, l + 64, ..: one float64 dot product per (candidate, cluster), summed over the columns in ascending
// order, and keeps the three best per candidate.  Three rounds of a wave arg-max merge the lanes' lists; lane 0 then walks the tuples.
// Every candidate picks among its (at most) three best clusters, or -1 when there are fewer clusters than candidates: at most 4^3 tuples, of
// which the valid ones (n = min(m, K) pairwise different clusters) are compared by their total, summed in slot order, then by the label
// tuple with -1 last.  Lane 0 alone leaves with the result: lab [3] (-1: none) and cosv [3], the float64 cosine to the label (0 for none).
__device__ __forceinline__ void assign_solve(AssignLds& L, const bool cand[3], const double* __restrict__ cent, int K, int d, int constrained,
                                             int lane, int32_t lab[3], double cosv[3]) {
  Top3 t[3];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int i = 0; i < 3; ++i) { t[s].v[i] = 0.0; t[s].k[i] = -1; }
  for (int k = lane; k < K; k += 64) {
    const double* ck = cent + (int64_t)k * d;
    double a[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < d; j += 2) {
      const double2 w = *reinterpret_cast<const double2*>(ck + j);
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (cand[s]) {
          a[s] = fma(L.e[s][j], w.x, a[s]);
          a[s] = fma(L.e[s][j + 1], w.y, a[s]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) if (cand[s]) top3_push(t[s], a[s], k);
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {                      // round r: the best head of the wave, popped from the lane that holds it
      double v = t[s].v[0];
      int k = t[s].k[0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int ok = __shfl_xor(k, o, 64);
        if (ok >= 0 && better(ov, ok, v, k)) { v = ov; k = ok; }
      }
      if (k >= 0 && k == t[s].k[0]) {
        t[s].v[0] = t[s].v[1]; t[s].k[0] = t[s].k[1]; t[s].v[1] = t[s].v[2]; t[s].k[1] = t[s].k[2]; t[s].k[2] = -1;
      }
      if (lane == 0) { L.v[s][r] = v; L.k[s][r] = k; }
    }
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) { lab[s] = -1; cosv[s] = 0.0; }
  if (lane != 0) return;
  int slot[3], m = 0;
#pragma unroll
  for (int s = 0; s < 3; ++s) if (cand[s]) slot[m++] = s;
  if (!constrained) {
    for (int i = 0; i < m; ++i) {
      const int s = slot[i];
      if (L.k[s][0] >= 0) { lab[s] = L.k[s][0]; cosv[s] = L.v[s][0]; }
    }
  } else if (m > 0) {
    const int n = min(m, K), nopt = K < m ? 4 : 3;     // option 3 of a candidate: no cluster (only when some candidate must go without)
    bool have = false;
    double best = 0.0;
    int bl[3] = {-1, -1, -1}, bo[3] = {0, 0, 0};
    const int total_tuples = m == 1 ? nopt : m == 2 ? nopt * nopt : nopt * nopt * nopt;
    for (int u = 0; u < total_tuples; ++u) {
      int o[3], l[3], used = 0;
      int rest = u;
      for (int i = m - 1; i >= 0; --i) { o[i] = rest % nopt; rest /= nopt; }      // slot 0 is the most significant digit
      bool ok = true;
      double tot = 0.0;
      for (int i = 0; i < m && ok; ++i) {
        l[i] = o[i] < 3 ? L.k[slot[i]][o[i]] : -1;
        if (o[i] < 3) {
          ok = l[i] >= 0;
          for (int p = 0; p < i; ++p) ok = ok && l[p] != l[i];
          if (ok) { tot += L.v[slot[i]][o[i]]; ++used; }
        }
      }
      if (!ok || used != n) continue;
      bool take = !have || tot > best;
      if (have && tot == best) {                       // the smaller label tuple in slot order, -1 after every cluster
        for (int i = 0; i < m; ++i) {
          const unsigned x = (unsigned)l[i], y = (unsigned)bl[i];               // -1 -> 0xffffffff
          if (x != y) { take = x < y; break; }
        }
      }
      if (take) {
        have = true;
        best = tot;
        for (int i = 0; i < m; ++i) { bl[i] = l[i]; bo[i] = o[i]; }
      }
    }
    if (have)
      for (int i = 0; i < m; ++i) {
        lab[slot[i]] = bl[i];
        cosv[slot[i]] = bl[i] >= 0 ? L.v[slot[i]][bo[i]] : 0.0;
      }
  }
}

}  // namespace
