// Verification trials: every (test row, model row) pair scored, classed and binned - the score matrix is never written (trials.py states the rule).
//
//   s(i, j) = r[j] + sum_k A[i][k] B[j][k]   float64;   t = (s - lo) * scale (one subtraction, one multiplication, never an FMA);
//   q = floor(t) in [0, 2^24), or below (t < 0), above (t >= 2^24, +inf included), nan;   bin = (q >> shift) - base.
//   trial (i, j): excluded when la[i] < 0 or lb[j] < 0 or (sa[i] >= 0 and sa[i] == sb[j]); else target (1) when la[i] == lb[j], else nontarget (0).
//
//   tr_hist_kernel       persistent workgroups; a workgroup owns a contiguous run of the 64 x 64 tiles of the [N, M] trial matrix (row-major over
//                        tiles, model tiles fastest: its A tile stays the same for a stretch while B streams), a function of (N, M) and the
//                        grid alone.  A tile is ps_score_kernel's product: four waves, each a 32 x 32 quadrant = 2 x 2 v_mfma_f64_16x16x4_f64
//                        tiles, A and B through LDS in chunks of 16 columns, the next chunk in flight in registers during the MFMAs (two
//                        stages: registers, then LDS).  Rows and columns outside the matrices are staged as zeros and are NOT counted.
//                        The epilogue works on the accumulator registers: class, exclusion and q per element, then
//                          - a trial whose bin lies in [0, 4096): ONE LDS integer atomic add (ds_add_u32, no return) into hist[class][bin]
//                            (2 x 4096 uint32, 32 KB);
//                          - under / over / nan / excluded: per-lane uint32 registers.  In a zoom pass all but one coarse bin's trials
//                            land there, so as LDS atomics they would be 64 lanes on one address for every element; in registers they are free.
//                        Flush: the LDS histogram and the wave-summed registers go to `out` with 64-bit integer global atomics, at the end and
//                        at least every TR_FLUSH_TILES tiles (a tile adds at most 4096 to a counter).
//
// Everything after the product is integer arithmetic; integer atomics commute: the counters do not depend on the grid, the tile order or the
// arrival order, and two runs agree bit for bit.  The product itself is one chain in one order per element, as in ps_score_kernel.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int TR_NT = 256;
constexpr int TR_BM = 64, TR_BN = 64;       // tile of the workgroup: test rows x model rows
constexpr int TR_KC = 16;                   // columns k staged per step
constexpr int TR_LD = 80;                   // LDS row pitch in doubles (plda_score.hip: rows k and k + 1 of a fragment read fall into different halves of the banks)
constexpr int TR_BINS = 4096;
constexpr int TR_Q_BITS = 24;
constexpr int TR_MAX_ROWS = 1 << 20;
constexpr int TR_MAX_K = 512;
constexpr int TR_DEFAULT_BLOCKS = 512;      // 256 CUs x 2 workgroups (53.5 KB of LDS each; three miss the CU's 160 KB by 512 bytes): the default grid, capped by the number of tiles
constexpr int TR_FLUSH_TILES = 1 << 19;     // tiles between two flushes of the LDS histogram
constexpr int TR_OUT = 2 * TR_BINS + 7;     // hist[2][4096], under[2], over[2], nan[2], excluded[1]

static_assert((uint64_t)TR_FLUSH_TILES * (uint64_t)(TR_BM * TR_BN) <= 0xffffffffull, "a uint32 counter cannot wrap between two flushes");
static_assert(2 * TR_KC * TR_LD * 8 + 2 * TR_BINS * 4 + 4 * 64 * 4 + 64 * 8 <= 65536, "static LDS of the kernel");

typedef double tr_d4 __attribute__((ext_vector_type(4)));
typedef double tr_d2 __attribute__((ext_vector_type(2)));

struct TrCount {
  uint32_t under[2], over[2], nan[2], excluded;
};

// HIST = false: the bench-only variant without the LDS atomics (in-range trials are counted per class in a register and land in bin 0)
template <bool HIST>
__global__ __launch_bounds__(TR_NT) void tr_hist_kernel(const double* __restrict__ A, int N, const double* __restrict__ B,
                                                        const double* __restrict__ r, int M, int K, const int32_t* __restrict__ la,
                                                        const int32_t* __restrict__ sa, const int32_t* __restrict__ lb,
                                                        const int32_t* __restrict__ sb, double lo, double scale, int shift, uint32_t base,
                                                        int ntn, int ntiles, unsigned long long* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double s_mem[2 * TR_KC * TR_LD];
  __shared__ uint32_t s_hist[2 * TR_BINS];
  __shared__ int32_t s_la[TR_BM], s_sa[TR_BM], s_lb[TR_BN], s_sb[TR_BN];
  __shared__ double s_r[TR_BN];
  double (*s_a)[TR_LD] = reinterpret_cast<double (*)[TR_LD]>(s_mem);                      // [TR_KC][TR_LD]: A[row][k] as [k][row]
  double (*s_b)[TR_LD] = reinterpret_cast<double (*)[TR_LD]>(s_mem + TR_KC * TR_LD);      // [TR_KC][TR_LD]: B[row][k] as [k][row]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = wave >> 1, qj = wave & 1, fk = lane >> 4, fc = lane & 15;
  // staging: thread = (row tid & 63 of the tile, columns 4 (tid >> 6) .. + 3 of the chunk)
  const int sr = tid & 63, sk = 4 * (tid >> 6);
  const int t0 = (int)((int64_t)blockIdx.x * ntiles / gridDim.x), t1 = (int)((int64_t)(blockIdx.x + 1) * ntiles / gridDim.x);
  for (int i = tid; i < 2 * TR_BINS; i += TR_NT) s_hist[i] = 0;       // before the first tile's barriers
  TrCount c = {{0, 0}, {0, 0}, {0, 0}, 0};
  uint32_t inr[2] = {0, 0};                                           // HIST = false only
  const tr_d2 zero2 = {0.0, 0.0};

  auto flush = [&]() {                                                // every wave's epilogue is done (a barrier precedes)
    for (int i = tid; i < 2 * TR_BINS; i += TR_NT) {
      const uint32_t v = s_hist[i];
      if (v) {
        atomicAdd(out + i, (unsigned long long)v);
        s_hist[i] = 0;
      }
    }
    uint32_t v[9] = {c.under[0], c.under[1], c.over[0], c.over[1], c.nan[0], c.nan[1], c.excluded, inr[0], inr[1]};
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = wave_sum(v[k]);             // at most 64 lanes x 2^19 tiles x 16 elements = 2^29
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (v[k]) atomicAdd(out + 2 * TR_BINS + k, (unsigned long long)v[k]);
      if (!HIST) {
        if (v[7]) atomicAdd(out, (unsigned long long)v[7]);
        if (v[8]) atomicAdd(out + TR_BINS, (unsigned long long)v[8]);
      }
    }
    c = TrCount{{0, 0}, {0, 0}, {0, 0}, 0};
    inr[0] = inr[1] = 0;
  };

  int since = 0;
  for (int tile = t0; tile < t1; ++tile) {
    const int row0 = (tile / ntn) * TR_BM, col0 = (tile % ntn) * TR_BN;
    const int64_t arow = row0 + sr, brow = col0 + sr;
    const bool aok = arow < N, bok = brow < M;
    tr_d2 ra[2], rb[2];
    auto fetch = [&](int d0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ra[h] = aok ? *reinterpret_cast<const tr_d2*>(A + arow * K + d0 + sk + 2 * h) : zero2;
        rb[h] = bok ? *reinterpret_cast<const tr_d2*>(B + brow * K + d0 + sk + 2 * h) : zero2;
      }
    };
    tr_d4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = tr_d4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    // the tile's labels, sessions and r: written after the first barrier (the previous tile's epilogue has read its own), read in the epilogue
    int32_t my_l = -1, my_s = -1;
    double my_r = 0.0;
    if (tid < 64) {
      if (aok) { my_l = la[arow]; my_s = sa[arow]; }
    } else if (tid < 128) {
      if (bok) { my_l = lb[brow]; my_s = sb[brow]; my_r = r[brow]; }
    }
    for (int d0 = 0; d0 < K; d0 += TR_KC) {
      __syncthreads();                                   // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          s_a[sk + 2 * h + e][sr] = ra[h][e];
          s_b[sk + 2 * h + e][sr] = rb[h][e];
        }
      if (d0 == 0) {
        if (tid < 64) { s_la[sr] = my_l; s_sa[sr] = my_s; }
        else if (tid < 128) { s_lb[sr] = my_l; s_sb[sr] = my_s; s_r[sr] = my_r; }
      }
      __syncthreads();
      if (d0 + TR_KC < K) fetch(d0 + TR_KC);             // in flight during the MFMAs
#pragma unroll
      for (int ks = 0; ks < TR_KC / 4; ++ks) {
        const int kk = ks * 4 + fk;
        const double a0 = s_a[kk][qi * 32 + fc], a1 = s_a[kk][qi * 32 + 16 + fc];
        const double b0 = s_b[kk][qj * 32 + fc], b1 = s_b[kk][qj * 32 + 16 + fc];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg.  Labels were written before this tile's last barrier.
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int lc = qj * 32 + v * 16 + fc;
      const bool cok = col0 + lc < M;
      const int32_t lbj = s_lb[lc], sbj = s_sb[lc];
      const double rj = s_r[lc];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lr = qi * 32 + u * 16 + fk + 4 * reg;
          if (!cok || row0 + lr >= N) continue;          // outside the matrices: not a trial
          const int32_t lai = s_la[lr], sai = s_sa[lr];
          if (lai < 0 || lbj < 0 || (sai >= 0 && sai == sbj)) {
            c.excluded += 1;
            continue;
          }
          const int cls = lai == lbj ? 1 : 0;
          const double s = acc[u][v][reg] + rj;
          const double t = __dmul_rn(__dsub_rn(s, lo), scale);
          if (t != t) {
            c.nan[cls] += 1;
          } else if (t < 0.0) {
            c.under[cls] += 1;
          } else if (t >= 16777216.0) {
            c.over[cls] += 1;
          } else {
            const uint32_t qs = (uint32_t)t >> shift;    // t in [0, 2^24): the conversion truncates = floor
            if (qs < base) {
              c.under[cls] += 1;
            } else if (qs - base >= (uint32_t)TR_BINS) {
              c.over[cls] += 1;
            } else if (HIST) {
              atomicAdd(&s_hist[cls * TR_BINS + (int)(qs - base)], 1u);
            } else {
              inr[cls] += 1;
            }
          }
        }
    }
    if (++since == TR_FLUSH_TILES) {
      __syncthreads();
      flush();
      since = 0;
    }
  }
  __syncthreads();
  flush();
}

// ---- calibration: the sums of the logistic objective over every trial (trials.py states the rule) -----------------------------------------------
//
//   tr_calib_kernel      tr_hist_kernel's persistent 64 x 64 tiling and product; the epilogue, on the accumulator registers, forms per trial
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
//
// The tile product below is a COPY of tr_hist_kernel's.  Written once as a __device__ __forceinline__ function called by both kernels, it
// changed tr_hist_kernel's register allocation (103 / 101 VGPRs for HIST = false / true became 99 / 97; SGPRs, AGPRs, scratch and LDS stayed):
// the histogram kernel is measured and pinned as it is, so it keeps its body and this kernel carries its own.
constexpr int TC_TERMS = 7;                 // loss, w, w s, v, v s, v s^2, s
constexpr int TC_ROW = 2 * (TC_TERMS + 1);  // a workgroup's row of partials: [2][8]
constexpr int TC_COUNTS = 5;                // n[2], nonfinite[2], excluded
constexpr int TC_DEFAULT_BLOCKS = 512;      // 256 CUs x 2 workgroups: the compiler gives 191 VGPRs + 32 AGPRs, no scratch, 2 waves / SIMD - the registers bind, not
                                            // the 22 KB of LDS (forced to 3 waves / SIMD it fits 168 VGPRs with 12 bytes of scratch per lane: not taken, unmeasured)

__global__ __launch_bounds__(TR_NT) void tr_calib_kernel(const double* __restrict__ A, int N, const double* __restrict__ B,
                                                         const double* __restrict__ r, int M, int K, const int32_t* __restrict__ la,
                                                         const int32_t* __restrict__ sa, const int32_t* __restrict__ lb,
                                                         const int32_t* __restrict__ sb, double ca, double cc, int ntn, int ntiles,
                                                         double* __restrict__ partials, unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) double s_mem[2 * TR_KC * TR_LD];
  __shared__ int32_t s_la[TR_BM], s_sa[TR_BM], s_lb[TR_BN], s_sb[TR_BN];
  __shared__ double s_r[TR_BN];
  __shared__ double s_red[4][2 * TC_TERMS];
  __shared__ unsigned long long s_cnt[4][2];
  double (*s_a)[TR_LD] = reinterpret_cast<double (*)[TR_LD]>(s_mem);                      // [TR_KC][TR_LD]: A[row][k] as [k][row]
  double (*s_b)[TR_LD] = reinterpret_cast<double (*)[TR_LD]>(s_mem + TR_KC * TR_LD);      // [TR_KC][TR_LD]: B[row][k] as [k][row]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = wave >> 1, qj = wave & 1, fk = lane >> 4, fc = lane & 15;
  // staging: thread = (row tid & 63 of the tile, columns 4 (tid >> 6) .. + 3 of the chunk)
  const int sr = tid & 63, sk = 4 * (tid >> 6);
  const int t0 = (int)((int64_t)blockIdx.x * ntiles / gridDim.x), t1 = (int)((int64_t)(blockIdx.x + 1) * ntiles / gridDim.x);
  const tr_d2 zero2 = {0.0, 0.0};
  double sum[2][TC_TERMS];
#pragma unroll
  for (int k = 0; k < TC_TERMS; ++k) sum[0][k] = sum[1][k] = 0.0;
  unsigned long long n[2] = {0, 0}, nonfinite[2] = {0, 0}, excluded = 0;      // 64 bits: one workgroup may own all 2^28 tiles

  for (int tile = t0; tile < t1; ++tile) {
    const int row0 = (tile / ntn) * TR_BM, col0 = (tile % ntn) * TR_BN;
    const int64_t arow = row0 + sr, brow = col0 + sr;
    const bool aok = arow < N, bok = brow < M;
    tr_d2 ra[2], rb[2];
    auto fetch = [&](int d0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ra[h] = aok ? *reinterpret_cast<const tr_d2*>(A + arow * K + d0 + sk + 2 * h) : zero2;
        rb[h] = bok ? *reinterpret_cast<const tr_d2*>(B + brow * K + d0 + sk + 2 * h) : zero2;
      }
    };
    tr_d4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = tr_d4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    // the tile's labels, sessions and r: written after the first barrier (the previous tile's epilogue has read its own), read in the epilogue
    int32_t my_l = -1, my_s = -1;
    double my_r = 0.0;
    if (tid < 64) {
      if (aok) { my_l = la[arow]; my_s = sa[arow]; }
    } else if (tid < 128) {
      if (bok) { my_l = lb[brow]; my_s = sb[brow]; my_r = r[brow]; }
    }
    for (int d0 = 0; d0 < K; d0 += TR_KC) {
      __syncthreads();                                   // the previous chunk's reads (and the previous tile's epilogue) are done
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          s_a[sk + 2 * h + e][sr] = ra[h][e];
          s_b[sk + 2 * h + e][sr] = rb[h][e];
        }
      if (d0 == 0) {
        if (tid < 64) { s_la[sr] = my_l; s_sa[sr] = my_s; }
        else if (tid < 128) { s_lb[sr] = my_l; s_sb[sr] = my_s; s_r[sr] = my_r; }
      }
      __syncthreads();
      if (d0 + TR_KC < K) fetch(d0 + TR_KC);             // in flight during the MFMAs
#pragma unroll
      for (int ks = 0; ks < TR_KC / 4; ++ks) {
        const int kk = ks * 4 + fk;
        const double a0 = s_a[kk][qi * 32 + fc], a1 = s_a[kk][qi * 32 + 16 + fc];
        const double b0 = s_b[kk][qj * 32 + fc], b1 = s_b[kk][qj * 32 + 16 + fc];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg.  Labels were written before this tile's last barrier.
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int lc = qj * 32 + v * 16 + fc;
      const bool cok = col0 + lc < M;
      const int32_t lbj = s_lb[lc], sbj = s_sb[lc];
      const double rj = s_r[lc];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lr = qi * 32 + u * 16 + fk + 4 * reg;
          if (!cok || row0 + lr >= N) continue;          // outside the matrices: not a trial
          const int32_t lai = s_la[lr], sai = s_sa[lr];
          if (lai < 0 || lbj < 0 || (sai >= 0 && sai == sbj)) {
            excluded += 1;
            continue;
          }
          const bool tgt = lai == lbj;
          const double s = acc[u][v][reg] + rj;
          if (!(fabs(s) < INFINITY)) {                   // NaN, +inf, -inf
            nonfinite[tgt ? 1 : 0] += 1;
            continue;
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
        }
    }
  }
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

static int tc_grid(int N, int M, int max_blocks, int64_t* tiles_out) {
  const int64_t tiles = (int64_t)ceil_div(N, TR_BM) * ceil_div(M, TR_BN);          // at most 2^28
  int grid = tiles < TC_DEFAULT_BLOCKS ? (int)tiles : TC_DEFAULT_BLOCKS;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (tiles_out) *tiles_out = tiles;
  return grid;
}

}  // namespace

extern "C" int sdk_trial_hist(sdk_ctx* ctx, const double* A, int N, const double* B, const double* r, int M, int K, const int32_t* la,
                              const int32_t* sa, const int32_t* lb, const int32_t* sb, double lo, double scale, int shift, int base, int max_blocks,
                              uint64_t* out, void* stream) {
  SDK_REQUIRE(K >= 16 && K <= TR_MAX_K && K % 16 == 0, "sdk_trial_hist: K=%d not supported (a multiple of 16 in 16 .. %d)", K, TR_MAX_K);
  SDK_REQUIRE(N >= 1 && N <= TR_MAX_ROWS && M >= 1 && M <= TR_MAX_ROWS, "sdk_trial_hist: N=%d test rows, M=%d model rows (1 .. %d each)", N, M,
              TR_MAX_ROWS);
  SDK_REQUIRE(shift >= 0 && shift <= TR_Q_BITS, "sdk_trial_hist: shift=%d (0 .. %d)", shift, TR_Q_BITS);
  SDK_REQUIRE(base >= 0 && base <= (1 << TR_Q_BITS), "sdk_trial_hist: base=%d (0 .. 2^%d)", base, TR_Q_BITS);
  SDK_REQUIRE(max_blocks >= 0, "sdk_trial_hist: max_blocks=%d (0: the default grid, else a cap on the workgroups)", max_blocks);
  SDK_REQUIRE(lo > -INFINITY && lo < INFINITY && scale > 0.0 && scale < INFINITY,
              "sdk_trial_hist: lo=%g scale=%g (lo finite, scale = 2^24 / (hi - lo) finite and above 0: lo < hi)", lo, scale);
  SDK_REQUIRE(ctx, "sdk_trial_hist: null context");
  SDK_REQUIRE(A && B && r && la && sa && lb && sb && out, "sdk_trial_hist: null argument (A=%p B=%p r=%p la=%p sa=%p lb=%p sb=%p out=%p)", (const void*)A,
              (const void*)B, (const void*)r, (const void*)la, (const void*)sa, (const void*)lb, (const void*)sb, (void*)out);
  SDK_REQUIRE((((uintptr_t)A | (uintptr_t)B) & 15) == 0, "sdk_trial_hist: A=%p and B=%p must be 16-byte aligned", (const void*)A, (const void*)B);
  SDK_REQUIRE(((uintptr_t)out & 7) == 0, "sdk_trial_hist: out=%p must be 8-byte aligned", (void*)out);
  const int ntm = ceil_div(N, TR_BM), ntn = ceil_div(M, TR_BN);
  const int64_t tiles = (int64_t)ntm * ntn;              // at most 2^28
  int grid = tiles < TR_DEFAULT_BLOCKS ? (int)tiles : TR_DEFAULT_BLOCKS;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * (double)M * K, 8.0 * (double)tiles * (TR_BM + TR_BN) * K);
  SDK_HIP_OK(hipMemsetAsync(out, 0, (size_t)TR_OUT * sizeof(uint64_t), st));
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  if (ctx->trials_no_hist)
    hipLaunchKernelGGL(tr_hist_kernel<false>, dim3(grid), dim3(TR_NT), 0, st, A, N, B, r, M, K, la, sa, lb, sb, lo, scale, shift, (uint32_t)base, ntn,
                       (int)tiles, o);
  else
    hipLaunchKernelGGL(tr_hist_kernel<true>, dim3(grid), dim3(TR_NT), 0, st, A, N, B, r, M, K, la, sa, lb, sb, lo, scale, shift, (uint32_t)base, ntn,
                       (int)tiles, o);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t sdk_trial_calib_workspace_bytes(int N, int M, int max_blocks) {
  if (!(N >= 1 && N <= TR_MAX_ROWS && M >= 1 && M <= TR_MAX_ROWS && max_blocks >= 0)) {
    sdk_set_error("sdk_trial_calib_workspace_bytes: N=%d M=%d max_blocks=%d (1 <= N, M <= %d, max_blocks at least 0)", N, M, max_blocks, TR_MAX_ROWS);
    return 0;
  }
  const size_t b = (size_t)tc_grid(N, M, max_blocks, nullptr) * TC_ROW * sizeof(double);
  return (b + 255) & ~(size_t)255;
}

extern "C" int sdk_trial_calib(sdk_ctx* ctx, const double* A, int N, const double* B, const double* r, int M, int K, const int32_t* la,
                               const int32_t* sa, const int32_t* lb, const int32_t* sb, double a, double c, int max_blocks, double* sums,
                               uint64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(K >= 16 && K <= TR_MAX_K && K % 16 == 0, "sdk_trial_calib: K=%d not supported (a multiple of 16 in 16 .. %d)", K, TR_MAX_K);
  SDK_REQUIRE(N >= 1 && N <= TR_MAX_ROWS && M >= 1 && M <= TR_MAX_ROWS, "sdk_trial_calib: N=%d test rows, M=%d model rows (1 .. %d each)", N, M,
              TR_MAX_ROWS);
  SDK_REQUIRE(max_blocks >= 0, "sdk_trial_calib: max_blocks=%d (0: the default grid, else a cap on the workgroups)", max_blocks);
  SDK_REQUIRE(a > -INFINITY && a < INFINITY && c > -INFINITY && c < INFINITY, "sdk_trial_calib: a=%g c=%g (the map z = a s + c: both finite)", a, c);
  SDK_REQUIRE(ctx, "sdk_trial_calib: null context");
  SDK_REQUIRE(A && B && r && la && sa && lb && sb && sums && counts,
              "sdk_trial_calib: null argument (A=%p B=%p r=%p la=%p sa=%p lb=%p sb=%p sums=%p counts=%p)", (const void*)A, (const void*)B,
              (const void*)r, (const void*)la, (const void*)sa, (const void*)lb, (const void*)sb, (void*)sums, (void*)counts);
  SDK_REQUIRE((((uintptr_t)A | (uintptr_t)B) & 15) == 0, "sdk_trial_calib: A=%p and B=%p must be 16-byte aligned", (const void*)A, (const void*)B);
  SDK_REQUIRE((((uintptr_t)sums | (uintptr_t)counts) & 7) == 0, "sdk_trial_calib: sums=%p and counts=%p must be 8-byte aligned", (void*)sums,
              (void*)counts);
  int64_t tiles = 0;
  const int grid = tc_grid(N, M, max_blocks, &tiles);
  const size_t need = (size_t)grid * TC_ROW * sizeof(double);
  SDK_REQUIRE(ws, "sdk_trial_calib: null workspace (%zu bytes needed, sdk_trial_calib_workspace_bytes)", need);
  SDK_REQUIRE(ws_bytes >= need, "sdk_trial_calib: workspace of %zu bytes, %zu needed (sdk_trial_calib_workspace_bytes)", ws_bytes, need);
  SDK_REQUIRE(((uintptr_t)ws & 255) == 0, "sdk_trial_calib: ws=%p must be 256-byte aligned", ws);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * N * (double)M * K, 8.0 * (double)tiles * (TR_BM + TR_BN) * K);
  SDK_HIP_OK(hipMemsetAsync(counts, 0, (size_t)TC_COUNTS * sizeof(uint64_t), st));
  double* partials = static_cast<double*>(ws);
  unsigned long long* cn = reinterpret_cast<unsigned long long*>(counts);
  hipLaunchKernelGGL(tr_calib_kernel, dim3(grid), dim3(TR_NT), 0, st, A, N, B, r, M, K, la, sa, lb, sb, a, c, ceil_div(M, TR_BN), (int)tiles, partials,
                     cn);
  SDK_LAUNCH_CHECK();
  hipLaunchKernelGGL(tr_calib_sum_kernel, dim3(1), dim3(64), 0, st, partials, grid, sums, cn);
  SDK_LAUNCH_CHECK();
  return 0;
}
