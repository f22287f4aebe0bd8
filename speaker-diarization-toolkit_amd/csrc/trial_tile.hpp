// The float64 trial tile shared by the verification-trial kernels (trials.hip: tr_hist_kernel, tr_calib_kernel; trials_snorm.hip:
// tr_hist_snorm_kernel): the constants, the walk over the [N, M] trial matrix with its product and exclusion rule, the histogram epilogue
// and the host-side checks of the entry points.  Each of these is written here once; a kernel adds its LDS, its per-row payload and its epilogue.
//
//   trial (i, j): excluded when la[i] < 0 or lb[j] < 0 or (sa[i] >= 0 and sa[i] == sb[j]); else target (1) when la[i] == lb[j], else nontarget (0).
//
//   tt_walk     persistent workgroups; a workgroup owns a contiguous run of the 64 x 64 tiles of the trial matrix (row-major over tiles, model
//               tiles fastest: its A tile stays the same for a stretch while B streams), a function of (N, M) and the grid alone.  A tile is
//               ps_score_kernel's product: four waves, each a 32 x 32 quadrant = 2 x 2 v_mfma_f64_16x16x4_f64 tiles, A and B through LDS in
//               chunks of 16 columns, the next chunk in flight in registers during the MFMAs (two stages: registers, then LDS).  Rows and
//               columns outside the matrices are staged as zeros, are never dereferenced and are NOT trials.  The product of a trial is one
//               chain in one order, whatever the grid.  Every live trial goes to the kernel's epilogue on the accumulator registers.
//   trial_bin   the histogram epilogue: a trial whose bin lies in [0, 4096) is ONE LDS integer atomic add (ds_add_u32, no return) into
//               hist[class][bin] (2 x 4096 uint32, 32 KB); under / over / nan / excluded are per-lane uint32 registers.  In a zoom pass all
//               but one coarse bin's trials land there, so as LDS atomics they would be 64 lanes on one address for every element; in
//               registers they are free.
//   tt_flush    the LDS histogram and the wave-summed registers go to `out` with 64-bit integer global atomics, at the end and at least every
//               TT_FLUSH_TILES tiles (a tile adds at most 4096 to a counter).  Integer atomics commute: the counters do not depend on the
//               grid, the tile order or the arrival order, and two runs agree bit for bit.
#pragma once

#include "common.hpp"

#include <math.h>
#include <stdio.h>

#include <initializer_list>

namespace {

constexpr int TT_NT = 256;
constexpr int TT_BM = 64, TT_BN = 64;       // tile of the workgroup: test rows x model rows
constexpr int TT_KC = 16;                   // columns k staged per step
constexpr int TT_LD = 80;                   // LDS row pitch in doubles (plda_score.hip: rows k and k + 1 of a fragment read fall into different halves of the banks)
constexpr int TT_BINS = 4096;
constexpr int TT_Q_BITS = 24;
constexpr int TT_MAX_ROWS = 1 << 20;
constexpr int TT_MAX_K = 512;
constexpr int TT_DEFAULT_BLOCKS = 512;      // 256 CUs x 2 workgroups (the histogram kernels: 53.5 and 55 KB of LDS, three miss the CU's 160 KB; tr_calib_kernel:
                                            // 186 VGPRs + 32 AGPRs): the default grid, capped by the number of tiles
constexpr int TT_FLUSH_TILES = 1 << 19;     // tiles between two flushes of the LDS histogram
constexpr int TT_OUT = 2 * TT_BINS + 7;     // hist[2][4096], under[2], over[2], nan[2], excluded[1]

typedef double tt_d4 __attribute__((ext_vector_type(4)));
typedef double tt_d2 __attribute__((ext_vector_type(2)));

// the LDS every trial kernel has: the two staged chunks and the tile's labels and sessions
struct TtTile {
  __attribute__((aligned(16))) double a[TT_KC][TT_LD];      // A[row][k] as [k][row]
  double b[TT_KC][TT_LD];                                   // B[row][k] as [k][row]
  int32_t la[TT_BM], sa[TT_BM], lb[TT_BN], sb[TT_BN];
};
constexpr int TT_HIST_LDS_BYTES = (int)sizeof(TtTile) + 2 * TT_BINS * 4;      // a histogram kernel's LDS without its payload

static_assert((uint64_t)TT_FLUSH_TILES * (uint64_t)(TT_BM * TT_BN) <= 0xffffffffull, "a uint32 counter cannot wrap between two flushes");
static_assert(sizeof(TtTile) == 2 * TT_KC * TT_LD * 8 + 4 * 64 * 4, "the tile's LDS has no padding");

struct TtMatrices {
  const double *A, *B;                      // [N][K] test rows, [M][K] model rows
  const int32_t *la, *sa, *lb, *sb;
  int N, M, K, ntn, ntiles;                 // ntn: model tiles per row of tiles
};

// Walks the workgroup's tiles.  P is the per-row payload beyond labels and sessions: load(model, row) reads it from global memory for a row
// inside the matrices (threads 0 .. 63 the test rows, model = false; threads 64 .. 127 the model rows), store(model, local row, p) puts it into
// the kernel's LDS after the tile's first barrier (the previous tile's epilogue has read its own).  column(lc) reads the payload of a model row
// back, once for the eight trials a lane has in that column.  epilogue(cls, s, lr, lc, col) gets every live trial of the tile: class, product,
// local row and column, the column's payload; `excluded` counts the others.  tile_done() runs after a tile's epilogue.
template <class P, class Excluded, class Load, class Store, class Column, class Epilogue, class TileDone>
__device__ __forceinline__ void tt_walk(const TtMatrices& x, TtTile& s, Excluded& excluded, Load load, Store store, Column column,
                                        Epilogue epilogue, TileDone tile_done) {
  const int N = x.N, M = x.M, K = x.K;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = wave >> 1, qj = wave & 1, fk = lane >> 4, fc = lane & 15;
  // staging: thread = (row tid & 63 of the tile, columns 4 (tid >> 6) .. + 3 of the chunk)
  const int sr = tid & 63, sk = 4 * (tid >> 6);
  const int t0 = (int)((int64_t)blockIdx.x * x.ntiles / gridDim.x), t1 = (int)((int64_t)(blockIdx.x + 1) * x.ntiles / gridDim.x);
  const tt_d2 zero2 = {0.0, 0.0};
  for (int tile = t0; tile < t1; ++tile) {
    const int row0 = (tile / x.ntn) * TT_BM, col0 = (tile % x.ntn) * TT_BN;
    const int64_t arow = row0 + sr, brow = col0 + sr;
    const bool aok = arow < N, bok = brow < M;
    tt_d2 ra[2], rb[2];
    auto fetch = [&](int d0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ra[h] = aok ? *reinterpret_cast<const tt_d2*>(x.A + arow * K + d0 + sk + 2 * h) : zero2;
        rb[h] = bok ? *reinterpret_cast<const tt_d2*>(x.B + brow * K + d0 + sk + 2 * h) : zero2;
      }
    };
    tt_d4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = tt_d4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    // a row outside the matrices is not dereferenced and its slots are never read (the epilogue below skips it)
    int32_t my_l = -1, my_s = -1;
    P my_p = P();
    if (tid < 64) {
      if (aok) { my_l = x.la[arow]; my_s = x.sa[arow]; my_p = load(false, arow); }
    } else if (tid < 128) {
      if (bok) { my_l = x.lb[brow]; my_s = x.sb[brow]; my_p = load(true, brow); }
    }
    for (int d0 = 0; d0 < K; d0 += TT_KC) {
      __syncthreads();                                   // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          s.a[sk + 2 * h + e][sr] = ra[h][e];
          s.b[sk + 2 * h + e][sr] = rb[h][e];
        }
      if (d0 == 0) {
        if (tid < 64) { s.la[sr] = my_l; s.sa[sr] = my_s; store(false, sr, my_p); }
        else if (tid < 128) { s.lb[sr] = my_l; s.sb[sr] = my_s; store(true, sr, my_p); }
      }
      __syncthreads();
      if (d0 + TT_KC < K) fetch(d0 + TT_KC);             // in flight during the MFMAs
#pragma unroll
      for (int ks = 0; ks < TT_KC / 4; ++ks) {
        const int kk = ks * 4 + fk;
        const double a0 = s.a[kk][qi * 32 + fc], a1 = s.a[kk][qi * 32 + 16 + fc];
        const double b0 = s.b[kk][qj * 32 + fc], b1 = s.b[kk][qj * 32 + 16 + fc];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg.  Labels and payload were written before this tile's last barrier.
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int lc = qj * 32 + v * 16 + fc;
      const bool cok = col0 + lc < M;
      const int32_t lbj = s.lb[lc], sbj = s.sb[lc];
      const auto col = column(lc);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lr = qi * 32 + u * 16 + fk + 4 * reg;
          if (!cok || row0 + lr >= N) continue;          // outside the matrices: not a trial
          const int32_t lai = s.la[lr], sai = s.sa[lr];
          if (lai < 0 || lbj < 0 || (sai >= 0 && sai == sbj)) {
            excluded += 1;
            continue;
          }
          epilogue(lai == lbj ? 1 : 0, acc[u][v][reg], lr, lc, col);
        }
    }
    tile_done();
  }
}

// ---- the histogram epilogue -----------------------------------------------------------------------------------------------------------------
struct TtCount {
  uint32_t under[2], over[2], nan[2], excluded;
  uint32_t inr[2];                          // HIST = false only: the in-range trials per class
};

__device__ __forceinline__ void tt_hist_clear(uint32_t* s_hist) {     // before the first tile's barriers
  for (int i = threadIdx.x; i < 2 * TT_BINS; i += TT_NT) s_hist[i] = 0;
}

// t = (score - lo) * scale of a live trial of class cls: q = floor(t) in [0, 2^24), or below (t < 0), above (t >= 2^24, +inf included), nan;
// bin = (q >> shift) - base.  HIST = false: the bench-only variant without the LDS atomics (in-range trials are counted per class in a register)
template <bool HIST = true>
__device__ __forceinline__ void trial_bin(double t, int cls, int shift, uint32_t base, uint32_t* s_hist, TtCount& c) {
  if (t != t) {
    c.nan[cls] += 1;
  } else if (t < 0.0) {
    c.under[cls] += 1;
  } else if (t >= 16777216.0) {
    c.over[cls] += 1;
  } else {
    const uint32_t qs = (uint32_t)t >> shift;            // t in [0, 2^24): the conversion truncates = floor
    if (qs < base) {
      c.under[cls] += 1;
    } else if (qs - base >= (uint32_t)TT_BINS) {
      c.over[cls] += 1;
    } else if (HIST) {
      atomicAdd(&s_hist[cls * TT_BINS + (int)(qs - base)], 1u);
    } else {
      c.inr[cls] += 1;
    }
  }
}

// every wave's epilogue is done (a barrier precedes).  HIST = false: the in-range trials land in bin 0 of their class
template <bool HIST = true>
__device__ __forceinline__ void tt_flush(uint32_t* s_hist, TtCount& c, unsigned long long* out) {
  for (int i = threadIdx.x; i < 2 * TT_BINS; i += TT_NT) {
    const uint32_t v = s_hist[i];
    if (v) {
      atomicAdd(out + i, (unsigned long long)v);
      s_hist[i] = 0;
    }
  }
  uint32_t v[9] = {c.under[0], c.under[1], c.over[0], c.over[1], c.nan[0], c.nan[1], c.excluded, c.inr[0], c.inr[1]};
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = wave_sum(v[k]);               // at most 64 lanes x 2^19 tiles x 16 elements = 2^29
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (v[k]) atomicAdd(out + 2 * TT_BINS + k, (unsigned long long)v[k]);
    if (!HIST) {
      if (v[7]) atomicAdd(out, (unsigned long long)v[7]);
      if (v[8]) atomicAdd(out + TT_BINS, (unsigned long long)v[8]);
    }
  }
  c = TtCount{{0, 0}, {0, 0}, {0, 0}, 0, {0, 0}};
}

// after a tile: a flush every TT_FLUSH_TILES tiles
template <bool HIST = true>
__device__ __forceinline__ void tt_flush_due(int& since, uint32_t* s_hist, TtCount& c, unsigned long long* out) {
  if (++since == TT_FLUSH_TILES) {
    __syncthreads();
    tt_flush<HIST>(s_hist, c, out);
    since = 0;
  }
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------------
// the grid of a trial kernel: one workgroup per tile up to the default, capped by max_blocks when it is above 0
static inline int tt_grid(int N, int M, int max_blocks, int64_t* tiles_out) {
  const int64_t tiles = (int64_t)ceil_div(N, TT_BM) * ceil_div(M, TT_BN);          // at most 2^28
  int grid = tiles < TT_DEFAULT_BLOCKS ? (int)tiles : TT_DEFAULT_BLOCKS;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (tiles_out) *tiles_out = tiles;
  return grid;
}

struct TtPtr {
  const char* name;
  const void* p;
};

// What every trial entry point requires: K, N, M, max_blocks, the context, no null among `ptrs` (the entry point's device pointers in the
// order of its message; the first two are A and B) and 16-byte aligned A and B.  0, or 2 with the error set.
static inline int tt_require(const char* who, sdk_ctx* ctx, int N, int M, int K, int max_blocks, std::initializer_list<TtPtr> ptrs) {
  SDK_REQUIRE(K >= 16 && K <= TT_MAX_K && K % 16 == 0, "%s: K=%d not supported (a multiple of 16 in 16 .. %d)", who, K, TT_MAX_K);
  SDK_REQUIRE(N >= 1 && N <= TT_MAX_ROWS && M >= 1 && M <= TT_MAX_ROWS, "%s: N=%d test rows, M=%d model rows (1 .. %d each)", who, N, M, TT_MAX_ROWS);
  SDK_REQUIRE(max_blocks >= 0, "%s: max_blocks=%d (0: the default grid, else a cap on the workgroups)", who, max_blocks);
  SDK_REQUIRE(ctx, "%s: null context", who);
  bool null = false;
  char list[512];
  int n = 0;
  for (const TtPtr& q : ptrs) {
    null = null || !q.p;
    n += snprintf(list + n, sizeof(list) - n, n ? " %s=%p" : "%s=%p", q.name, q.p);
  }
  SDK_REQUIRE(!null, "%s: null argument (%s)", who, list);
  const void *A = ptrs.begin()[0].p, *B = ptrs.begin()[1].p;
  SDK_REQUIRE((((uintptr_t)A | (uintptr_t)B) & 15) == 0, "%s: A=%p and B=%p must be 16-byte aligned", who, A, B);
  return 0;
}

// the score range of a histogram pass
static inline int tt_require_range(const char* who, double lo, double scale, int shift, int base) {
  SDK_REQUIRE(shift >= 0 && shift <= TT_Q_BITS, "%s: shift=%d (0 .. %d)", who, shift, TT_Q_BITS);
  SDK_REQUIRE(base >= 0 && base <= (1 << TT_Q_BITS), "%s: base=%d (0 .. 2^%d)", who, base, TT_Q_BITS);
  SDK_REQUIRE(lo > -INFINITY && lo < INFINITY && scale > 0.0 && scale < INFINITY,
              "%s: lo=%g scale=%g (lo finite, scale = 2^24 / (hi - lo) finite and above 0: lo < hi)", who, lo, scale);
  return 0;
}

}  // namespace
