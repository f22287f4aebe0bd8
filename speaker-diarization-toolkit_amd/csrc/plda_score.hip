// PLDA log-likelihood-ratio scoring of windows against enrolled SPEAKERS (plda_score.py states the rule): the per-speaker table and the top-k.
// Float64 throughout, in the diagonalised space of sdk_plda_transform (within-speaker covariance I, between-speaker covariance diag(Phi)).
//
//   llr(x, s) = r_s + sum_d x_d G[s][d] + sum_d x_d^2 G[s][D + d],   G[s] = [g(n_s) o u_s, q(n_s)],   r_s = c(n_s) + sum_d u_sd^2 h_d(n_s)
//
//   pe_count_kernel / pe_offsets_kernel / pe_fill_kernel    the rows of every speaker: integer counts (atomics on integers are exact in any
//                        order), their exclusive scan, and the row indices dealt into the speakers' segments in ANY order.  A label outside
//                        [0, S) is counted nowhere, dealt nowhere and sets status bit 1.
//   pe_pool_kernel       wave = speaker.  The segment is walked in ASCENDING row order whatever order it was dealt in: each step takes the
//                        least row index above the last one (a wave-wide minimum), so the walk costs m^2 / 64 index reads for m rows - meant
//                        for speakers of a few to a few hundred enrolments, correct and slow beyond.  u = (sum of the rows) / m; then the
//                        coefficients per column and r = the columns' terms, lane l adding columns l and l + 64, the lanes in a fixed
//                        xor tree.  A speaker without a row, or whose n_eff is not a finite positive number: G row of zeros, r = NaN.
//   ps_score_kernel      grid (speaker splits, tiles of 64 windows).  A workgroup walks its split's tiles of 64 speakers; a tile of the score
//                        matrix is a GEMM of depth 2 D on v_mfma_f64_16x16x4_f64: four waves, each a 32 x 32 quadrant = 2 x 2 MFMA tiles.  X and
//                        G pass through LDS in chunks of 16 columns d (x and x^2 = x * x, formed while staging: Z = [x, x^2] never exists in
//                        memory; G's columns d and D + d), the next chunk in flight in registers meanwhile.  Every score is ONE chain in ONE
//                        order - per chunk of 16 columns the 16 x-terms, then the 16 x^2-terms, four terms per MFMA - plus r_s, rows and
//                        columns outside the matrices are zeros: a score does not depend on its tile, its split, N or S.  The tile is parked in
//                        LDS (over the staging buffers); thread (window, quarter of the tile's columns) keeps a running top-4; the quarters
//                        merge at the end.  One split: the workgroup writes idx / score.  Several: it writes its list to the workspace.
//   ps_merge_kernel      thread = window: the splits' lists in split order.  "Better" is a strict total order (larger score, then lower
//                        speaker), so the k best do not depend on the tiling or the splitting; a NaN never enters a list.
//
// No floating-point atomics; one owner per output element; every sum in a fixed order: two runs agree bit for bit.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int PS_NT = 256;
constexpr int PS_BM = 64, PS_BN = 64;       // tile of the workgroup: windows x speakers
constexpr int PS_KC = 16;                   // columns d staged per step (32 terms of the chain: x and x^2)
constexpr int PS_LD = 80;                   // LDS row pitch in doubles: rows k and k + 1 of a fragment read fall into different halves of the banks
constexpr int PS_SLD = PS_BN + 1;           // pitch of the parked tile
constexpr int PS_MAX_TOPK = 4;
constexpr int PS_MAX_S = 1 << 20;
constexpr int PS_MAX_P = 1 << 22;
constexpr int PS_MAX_N = 65536;
constexpr int PS_MIN_SPLIT_TILES = 4;       // a split is at least 256 speakers wide (unless S is smaller) ..
constexpr int PS_TARGET_BLOCKS = 1024;      // .. and there are about this many workgroups when S allows it: a function of (N, S) alone
constexpr int PS_ST_LABEL = 1;
constexpr int PS_LDS_DOUBLES = 2 * 2 * PS_KC * PS_LD;      // the two staging buffers; the parked tile and the quarters' lists lie over them

static_assert(PS_BM * PS_SLD <= PS_LDS_DOUBLES, "the parked tile lies over the staging buffers");
static_assert(PS_NT * PS_MAX_TOPK * 12 <= PS_LDS_DOUBLES * 8, "the quarters' lists lie over the staging buffers");

typedef double ps_d4 __attribute__((ext_vector_type(4)));
typedef double ps_d2 __attribute__((ext_vector_type(2)));

// ---- enrolment: the speaker table ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_NT) void pe_count_kernel(const int32_t* __restrict__ group, int P, int S, int32_t* __restrict__ counts,
                                                         int32_t* __restrict__ status) {
  const int p = blockIdx.x * PS_NT + threadIdx.x;
  if (p >= P) return;
  const int g = group[p];
  if ((unsigned)g < (unsigned)S) atomicAdd(counts + g, 1);
  else atomicOr(status, PS_ST_LABEL);
}

// one block, in place: off [0 .. S) holds the counts on entry; on return off [S + 1] = their exclusive scan and cursor [S] = off [0 .. S)
__global__ __launch_bounds__(1024) void pe_offsets_kernel(int32_t* off, int S, int32_t* __restrict__ cursor) {
  __shared__ int32_t s_part[1024];
  const int t = threadIdx.x, per = (S + 1023) / 1024;
  const int a = min(S, t * per), e = min(S, a + per);           // a thread's own entries: nobody else reads or writes them
  int32_t s = 0;
  for (int k = a; k < e; ++k) s += off[k];
  s_part[t] = s;
  __syncthreads();
  if (t == 0) {
    int32_t run = 0;
    for (int i = 0; i < 1024; ++i) {
      const int32_t v = s_part[i];
      s_part[i] = run;
      run += v;
    }
    off[S] = run;
  }
  __syncthreads();
  int32_t run = s_part[t];
  for (int k = a; k < e; ++k) {
    const int32_t c = off[k];
    off[k] = run;
    cursor[k] = run;
    run += c;
  }
}

__global__ __launch_bounds__(PS_NT) void pe_fill_kernel(const int32_t* __restrict__ group, int P, int S, int32_t* __restrict__ cursor,
                                                        int32_t* __restrict__ rows) {
  const int p = blockIdx.x * PS_NT + threadIdx.x;
  if (p >= P) return;
  const int g = group[p];
  if ((unsigned)g >= (unsigned)S) return;
  const int at = atomicAdd(cursor + g, 1);               // below off[g + 1] <= P: the counts hold exactly these rows
  rows[at] = p;
}

template <int D>
__global__ __launch_bounds__(PS_NT) void pe_pool_kernel(const double* __restrict__ Xp, int P, const int32_t* __restrict__ off,
                                                        const int32_t* __restrict__ rows, const double* __restrict__ n_eff,
                                                        const double* __restrict__ Phi, int S, double* __restrict__ G, double* __restrict__ r) {
  constexpr int NC = D / 64;                             // columns per lane: lane, lane + 64
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (PS_NT / 64) + (threadIdx.x >> 6);
  if (s >= S) return;                                    // wave-uniform
  const int p0 = off[s], m = off[s + 1] - p0;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  int last = -1;
  for (int t = 0; t < m; ++t) {
    int best = 0x7fffffff;
    for (int j = lane; j < m; j += 64) {
      const int v = rows[p0 + j];
      if (v > last && v < best) best = v;
    }
    best = wave_min(best);
    if ((unsigned)best >= (unsigned)P) break;            // cannot happen (m distinct rows in [0, P)); never an index outside Xp
    last = best;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += Xp[(int64_t)best * D + lane + 64 * c];
  }
  const double n = n_eff[s];
  const bool ok = m > 0 && n > 0.0 && n < INFINITY;      // a NaN fails both comparisons
  double term = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = lane + 64 * c;
    double g = 0.0, q = 0.0;
    if (ok) {
      const double phi = Phi[d], u = acc[c] / (double)m;
      const double den = n * phi + 1.0;
      const double a = n * phi / den, v = 1.0 + phi / den;
      g = a / v * u;
      q = -0.5 * (1.0 / v - 1.0 / (1.0 + phi));
      const double h = -(a * a) / (2.0 * v);
      term += -0.5 * (log(v) - log(1.0 + phi)) + u * u * h;
    }
    G[(int64_t)s * (2 * D) + d] = g;
    G[(int64_t)s * (2 * D) + D + d] = q;
  }
  term = wave_sum(term);
  if (lane == 0) r[s] = ok ? term : (double)NAN;
}

// ---- scoring ---------------------------------------------------------------------------------------------------------------------------
// a window's best entries, best first; idx < 0: empty
struct PsTop {
  double z[PS_MAX_TOPK];
  int idx[PS_MAX_TOPK];
};
__device__ __forceinline__ bool ps_better(double z, int i, double bz, int bi) { return bi < 0 || z > bz || (z == bz && i < bi); }
__device__ __forceinline__ void ps_push(PsTop& t, double z, int i) {
  if (!(z == z)) return;                                 // a NaN never wins
#pragma unroll
  for (int s = 0; s < PS_MAX_TOPK; ++s) {
    if (ps_better(z, i, t.z[s], t.idx[s])) {
      const double oz = t.z[s];
      const int oi = t.idx[s];
      t.z[s] = z; t.idx[s] = i;
      z = oz; i = oi;
      if (i < 0) return;
    }
  }
}
__device__ __forceinline__ void ps_clear(PsTop& t) {
#pragma unroll
  for (int s = 0; s < PS_MAX_TOPK; ++s) { t.z[s] = 0.0; t.idx[s] = -1; }
}
// the final answer of window n: columns S .. k - 1 are not written
__device__ __forceinline__ void ps_write(const PsTop& t, int64_t n, int k, int S, int32_t* __restrict__ idx, double* __restrict__ score) {
  const int kw = k < S ? k : S;
#pragma unroll
  for (int s = 0; s < PS_MAX_TOPK; ++s) {
    if (s >= kw) break;
    const bool have = t.idx[s] >= 0;
    idx[n * k + s] = have ? t.idx[s] : -1;
    score[n * k + s] = have ? t.z[s] : 0.0;
  }
}

// the speaker tiles and splits of (N, S): a function of the two alone
struct PsPlan {
  int ntn, nts, tps, nsplit;
};
inline PsPlan ps_plan(int N, int S) {
  PsPlan p;
  p.ntn = N < 1 ? 1 : ceil_div(N, PS_BM);
  p.nts = ceil_div(S, PS_BN);
  const int want = ceil_div(PS_TARGET_BLOCKS, p.ntn);
  p.tps = ceil_div(p.nts, want);
  if (p.tps < PS_MIN_SPLIT_TILES) p.tps = PS_MIN_SPLIT_TILES;
  p.nsplit = ceil_div(p.nts, p.tps);
  return p;
}

template <int D>
__global__ __launch_bounds__(PS_NT) void ps_score_kernel(const double* __restrict__ X, int N, const double* __restrict__ G,
                                                         const double* __restrict__ r, int S, int k, int tps, int32_t* __restrict__ idx,
                                                         double* __restrict__ score, double* __restrict__ scores, int32_t* __restrict__ pidx,
                                                         double* __restrict__ pscore) {
  __shared__ __attribute__((aligned(16))) double s_mem[PS_LDS_DOUBLES];
  double (*s_a)[PS_LD] = reinterpret_cast<double (*)[PS_LD]>(s_mem);                          // [2 PS_KC][PS_LD]: x, then x^2
  double (*s_b)[PS_LD] = reinterpret_cast<double (*)[PS_LD]>(s_mem + 2 * PS_KC * PS_LD);      // [2 PS_KC][PS_LD]: G[.][d], then G[.][D + d]
  double (*Ss)[PS_SLD] = reinterpret_cast<double (*)[PS_SLD]>(s_mem);                         // the parked tile, over both
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = wave >> 1, qj = wave & 1, fk = lane >> 4, fc = lane & 15;
  const int row0 = blockIdx.y * PS_BM;
  const int tile0 = blockIdx.x * tps, tile1 = min(tile0 + tps, (S + PS_BN - 1) / PS_BN);
  // staging: thread = (row tid & 63 of the tile, columns 4 (tid >> 6) .. + 3 of the chunk)
  const int sr = tid & 63, sk = 4 * (tid >> 6);
  const int64_t xrow = row0 + sr;
  const bool xok = xrow < N;
  // the top-k: thread = (window tid >> 2 of the tile, columns 16 (tid & 3) .. + 15 of the tile)
  const int lrow = tid >> 2, part = tid & 3;
  const bool live = row0 + lrow < N;
  PsTop top;
  ps_clear(top);
  const ps_d2 zero2 = {0.0, 0.0};
  for (int tile = tile0; tile < tile1; ++tile) {
    const int col0 = tile * PS_BN;
    const int64_t grow = col0 + sr;
    const bool gok = grow < S;
    ps_d2 ra[2], rg[2], rq[2];
    auto fetch = [&](int d0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ra[h] = xok ? *reinterpret_cast<const ps_d2*>(X + xrow * D + d0 + sk + 2 * h) : zero2;
        rg[h] = gok ? *reinterpret_cast<const ps_d2*>(G + grow * (2 * D) + d0 + sk + 2 * h) : zero2;
        rq[h] = gok ? *reinterpret_cast<const ps_d2*>(G + grow * (2 * D) + D + d0 + sk + 2 * h) : zero2;
      }
    };
    ps_d4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = ps_d4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int d0 = 0; d0 < D; d0 += PS_KC) {
      __syncthreads();                                   // the previous chunk's reads (and the previous tile's scan of Ss) are done
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const double x = ra[h][e];
          s_a[sk + 2 * h + e][sr] = x;
          s_a[PS_KC + sk + 2 * h + e][sr] = x * x;
          s_b[sk + 2 * h + e][sr] = rg[h][e];
          s_b[PS_KC + sk + 2 * h + e][sr] = rq[h][e];
        }
      __syncthreads();
      if (d0 + PS_KC < D) fetch(d0 + PS_KC);             // in flight during the MFMAs
#pragma unroll
      for (int ks = 0; ks < 2 * PS_KC / 4; ++ks) {
        const int kk = ks * 4 + fk;
        const double a0 = s_a[kk][qi * 32 + fc], a1 = s_a[kk][qi * 32 + 16 + fc];
        const double b0 = s_b[kk][qj * 32 + fc], b1 = s_b[kk][qj * 32 + 16 + fc];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    __syncthreads();                                     // the staging buffers are free: the tile goes over them
    // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int lc = qj * 32 + v * 16 + fc, col = col0 + lc;
      const double rs = col < S ? r[col] : 0.0;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lr = qi * 32 + u * 16 + fk + 4 * reg;
          const double val = acc[u][v][reg] + rs;
          Ss[lr][lc] = val;
          if (scores && row0 + lr < N && col < S) scores[(int64_t)(row0 + lr) * S + col] = val;
        }
    }
    __syncthreads();
    if (live) {
      for (int c = part * 16; c < part * 16 + 16; ++c) {
        const int col = col0 + c;
        if (col >= S) break;
        ps_push(top, Ss[lrow][c], col);
      }
    }
  }
  __syncthreads();                                       // the LDS becomes the lists of the four quarters of every window
  double* lz = s_mem;
  int* li = reinterpret_cast<int*>(s_mem + PS_NT * PS_MAX_TOPK);
#pragma unroll
  for (int s = 0; s < PS_MAX_TOPK; ++s) {
    lz[tid * PS_MAX_TOPK + s] = top.z[s];
    li[tid * PS_MAX_TOPK + s] = top.idx[s];
  }
  __syncthreads();
  if (!live || part != 0) return;
  for (int p = 1; p < 4; ++p)
#pragma unroll
    for (int s = 0; s < PS_MAX_TOPK; ++s) {
      const int o = (tid + p) * PS_MAX_TOPK + s;
      if (li[o] >= 0) ps_push(top, lz[o], li[o]);
    }
  const int64_t n = row0 + lrow;
  if (!pidx) {
    ps_write(top, n, k, S, idx, score);
    return;
  }
  const int64_t base = ((int64_t)blockIdx.x * N + n) * PS_MAX_TOPK;
#pragma unroll
  for (int s = 0; s < PS_MAX_TOPK; ++s) {
    pidx[base + s] = top.idx[s];
    pscore[base + s] = top.z[s];
  }
}

__global__ __launch_bounds__(PS_NT) void ps_merge_kernel(const int32_t* __restrict__ pidx, const double* __restrict__ pscore, int nsplit, int N,
                                                         int S, int k, int32_t* __restrict__ idx, double* __restrict__ score) {
  const int64_t n = (int64_t)blockIdx.x * PS_NT + threadIdx.x;
  if (n >= N) return;
  PsTop top;
  ps_clear(top);
  for (int sp = 0; sp < nsplit; ++sp) {
    const int64_t base = ((int64_t)sp * N + n) * PS_MAX_TOPK;
#pragma unroll
    for (int s = 0; s < PS_MAX_TOPK; ++s) {
      const int i = pidx[base + s];
      if (i >= 0 && i < S) ps_push(top, pscore[base + s], i);
    }
  }
  ps_write(top, n, k, S, idx, score);
}

// the score workspace: the splits' lists, scores [nsplit][N][4] float64 then indices [nsplit][N][4] int32 (nothing with one split)
struct PsWs {
  double* pscore;
  int32_t* pidx;
};
inline size_t ps_carve(WsCarver c, int N, int S, PsWs* w) {
  const PsPlan p = ps_plan(N, S);
  const size_t e = p.nsplit > 1 && N > 0 ? (size_t)p.nsplit * (size_t)N * PS_MAX_TOPK : 0;
  w->pscore = c.take<double>(e);
  w->pidx = c.take<int32_t>(e);
  return c.bytes();
}

// the enrolment workspace: off [S + 1], cursor [S], rows [P], int32
struct PeWs {
  int32_t *off, *cursor, *rows;
};
inline size_t pe_carve(WsCarver c, int P, int S, PeWs* w) {
  w->off = c.take<int32_t>((size_t)S + 1);
  w->cursor = c.take<int32_t>((size_t)S);
  w->rows = c.take<int32_t>((size_t)(P < 1 ? 1 : P));
  return c.bytes();
}

#define PS_REQUIRE_D(fn, D) SDK_REQUIRE((D) == 64 || (D) == 128, fn ": D=%d not supported (64 or 128)", (D))
#define PS_REQUIRE_S(fn, S) SDK_REQUIRE((S) >= 1 && (S) <= PS_MAX_S, fn ": S=%d speakers (1 .. %d)", (S), PS_MAX_S)

}  // namespace

extern "C" size_t sdk_plda_enroll_workspace_bytes(int P, int S) {
  if (!(P >= 0 && P <= PS_MAX_P && S >= 1 && S <= PS_MAX_S)) {
    sdk_set_error("sdk_plda_enroll_workspace_bytes: P=%d S=%d (0 <= P <= %d, 1 <= S <= %d)", P, S, PS_MAX_P, PS_MAX_S);
    return 0;
  }
  PeWs w;
  return pe_carve({}, P, S, &w);
}

extern "C" int sdk_plda_enroll(sdk_ctx* ctx, const double* Xp, const int32_t* group, int P, int D, const double* n_eff, const double* Phi, int S,
                               double* G, double* r, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  PS_REQUIRE_D("sdk_plda_enroll", D);
  PS_REQUIRE_S("sdk_plda_enroll", S);
  SDK_REQUIRE(P >= 0 && P <= PS_MAX_P, "sdk_plda_enroll: P=%d rows (0 .. %d)", P, PS_MAX_P);
  SDK_REQUIRE(ctx, "sdk_plda_enroll: null context");
  SDK_REQUIRE((P == 0 || (Xp && group)) && n_eff && Phi && G && r && status && ws,
              "sdk_plda_enroll: null argument (Xp=%p group=%p n_eff=%p Phi=%p G=%p r=%p status=%p ws=%p)", (const void*)Xp, (const void*)group,
              (const void*)n_eff, (const void*)Phi, (void*)G, (void*)r, (void*)status, ws);
  SDK_REQUIRE_WS("sdk_plda_enroll", "sdk_plda_enroll_workspace_bytes", ws, ws_bytes, sdk_plda_enroll_workspace_bytes(P, S), 256);
  PeWs w;
  pe_carve({static_cast<char*>(ws), 0}, P, S, &w);
  int32_t *const off = w.off, *const cursor = w.cursor, *const rows = w.rows;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 8.0 * ((double)P * D + 2.0 * (double)S * D) + 4.0 * (3.0 * P + 3.0 * S));
  SDK_HIP_OK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  SDK_HIP_OK(hipMemsetAsync(off, 0, ((size_t)S + 1) * sizeof(int32_t), st));        // the counts, until pe_offsets_kernel scans them in place
  if (P > 0) hipLaunchKernelGGL(pe_count_kernel, dim3(ceil_div(P, PS_NT)), dim3(PS_NT), 0, st, group, P, S, off, status);
  hipLaunchKernelGGL(pe_offsets_kernel, dim3(1), dim3(1024), 0, st, off, S, cursor);
  if (P > 0) hipLaunchKernelGGL(pe_fill_kernel, dim3(ceil_div(P, PS_NT)), dim3(PS_NT), 0, st, group, P, S, cursor, rows);
  const dim3 grid(ceil_div(S, PS_NT / 64));
  if (D == 64) hipLaunchKernelGGL(pe_pool_kernel<64>, grid, dim3(PS_NT), 0, st, Xp, P, (const int32_t*)off, (const int32_t*)rows, n_eff, Phi, S, G, r);
  else hipLaunchKernelGGL(pe_pool_kernel<128>, grid, dim3(PS_NT), 0, st, Xp, P, (const int32_t*)off, (const int32_t*)rows, n_eff, Phi, S, G, r);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t sdk_plda_score_workspace_bytes(int N, int S, int k) {
  if (!(N >= 0 && N <= PS_MAX_N && S >= 1 && S <= PS_MAX_S && k >= 1 && k <= PS_MAX_TOPK)) {
    sdk_set_error("sdk_plda_score_workspace_bytes: N=%d S=%d k=%d (0 <= N <= %d, 1 <= S <= %d, 1 <= k <= %d)", N, S, k, PS_MAX_N, PS_MAX_S,
                  PS_MAX_TOPK);
    return 0;
  }
  PsWs w;
  const size_t b = ps_carve({}, N, S, &w);
  return b ? b : 256;                                    // never 0 for arguments the call takes: 0 is the refusal
}

extern "C" int sdk_plda_score_topk(sdk_ctx* ctx, const double* X, int N, int D, const double* G, const double* r, int S, int k, int32_t* idx,
                                   double* score, double* scores, void* ws, size_t ws_bytes, void* stream) {
  PS_REQUIRE_D("sdk_plda_score_topk", D);
  PS_REQUIRE_S("sdk_plda_score_topk", S);
  SDK_REQUIRE(k >= 1 && k <= PS_MAX_TOPK, "sdk_plda_score_topk: k=%d (1 .. %d)", k, PS_MAX_TOPK);
  SDK_REQUIRE(N >= 0 && N <= PS_MAX_N, "sdk_plda_score_topk: N=%d windows (0 .. %d)", N, PS_MAX_N);
  SDK_REQUIRE(ctx, "sdk_plda_score_topk: null context");
  if (N == 0) return 0;
  SDK_REQUIRE(X && G && r && idx && score, "sdk_plda_score_topk: null argument (X=%p G=%p r=%p idx=%p score=%p)", (const void*)X, (const void*)G,
              (const void*)r, (void*)idx, (void*)score);
  SDK_REQUIRE((((uintptr_t)X | (uintptr_t)G) & 15) == 0, "sdk_plda_score_topk: X=%p and G=%p must be 16-byte aligned", (const void*)X, (const void*)G);
  const PsPlan plan = ps_plan(N, S);
  PsWs w{nullptr, nullptr};
  if (plan.nsplit > 1) {
    SDK_REQUIRE_WS("sdk_plda_score_topk", "sdk_plda_score_workspace_bytes", ws, ws_bytes, sdk_plda_score_workspace_bytes(N, S, k), 256);
    ps_carve({static_cast<char*>(ws), 0}, N, S, &w);
  }
  int32_t* const pidx = w.pidx;
  double* const pscore = w.pscore;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 4.0 * N * (double)S * D,
               8.0 * ((double)N * D + (double)plan.ntn * S * (2.0 * D + 1.0) + (scores ? (double)N * S : 0.0)) + 12.0 * N * k);
  const dim3 grid(plan.nsplit, plan.ntn);
  if (D == 64) hipLaunchKernelGGL(ps_score_kernel<64>, grid, dim3(PS_NT), 0, st, X, N, G, r, S, k, plan.tps, idx, score, scores, pidx, pscore);
  else hipLaunchKernelGGL(ps_score_kernel<128>, grid, dim3(PS_NT), 0, st, X, N, G, r, S, k, plan.tps, idx, score, scores, pidx, pscore);
  SDK_LAUNCH_CHECK();
  if (plan.nsplit > 1) {
    hipLaunchKernelGGL(ps_merge_kernel, dim3(ceil_div(N, PS_NT)), dim3(PS_NT), 0, st, (const int32_t*)pidx, (const double*)pscore, plan.nsplit, N, S, k, idx,
                       score);
    SDK_LAUNCH_CHECK();
  }
  return 0;
}
