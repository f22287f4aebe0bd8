// k6 (threshold path): centroid-linkage agglomerative clustering of G independent problems, float64 throughout, in scipy's layout and numbering
// (scipy.cluster.hierarchy.linkage(X, "centroid")).  Problem g is rows offsets[g] .. offsets[g+1] of one fp32 [N_total, dim] matrix.
//
//   ahc_table_kernel : the per-problem table (rows, workspace offsets, tile prefix) written into the workspace from kernel arguments
//   ahc_dist_kernel  : many workgroups, 64 x 64 tiles of the upper triangle of every problem: D[i][j] = D[j][i] = sqrt(sum_c (e_ic - e_jc)^2)
//                      in float64, difference form (2 - 2 e_i.e_j cancels at the small distances where merges happen); a non-finite
//                      distance (a NaN / Inf row: its own diagonal entry is NaN) sets status[g] = 1
//   ahc_nn_kernel    : one wave per row: nn[i] = argmin_{j > i} D[i][j] (ties -> lowest j), nnd[i] = that distance (+inf for the last row)
//   ahc_merge_kernel : one workgroup per problem, exactly n - 1 merges of Muellner's generic algorithm (scipy's fast_linkage), nnd kept as
//                      lower bounds checked lazily: argmin of the live rows' nnd (ties -> lowest row) = (x, y = nn[x]), accepted when
//                      D[x][y] equals it, else row x is rescanned and the search repeats; emit Z; Lance-Williams update of row and column y;
//                      a smaller new distance (or an equal one to a lower slot) lowers a bound; a row that pointed at x keeps its bound
//                      and holds NO neighbour (nn = -1) until it is the least and is rescanned; rescan row y.  Slot x dies, the merged
//                      cluster takes slot y and id n + t.  The pair of every step is therefore the live pair of least distance with ties
//                      to the lowest row slot, then the lowest neighbour, whatever the history.  (scipy guesses y for a row that pointed
//                      at x; a guess that happens to sit at the kept bound is accepted although a lower slot may sit there too, which
//                      made the tree of tied inputs depend on the order of earlier merges.)
//                      (Rescanning every row whose neighbour was x or y at once costs O(n) rescans per
//                      merge when many rows point at one growing cluster: tight clusters of 10^4 rows took minutes that way.)  Only
//                      __syncthreads inside the workgroup: nothing waits on another workgroup.
//
// Linked centroid linkage (sdk_linked_linkage; the LINK instantiations of the dist and merge kernels) - the rule:
//   input    unit rows E [N, d] fp32, group [N] int32, problems by offsets as above, stop: a float64 >= 0 or +inf
//   forbidden rows i != j of a problem are forbidden to each other when group[i] == group[j] >= 0 (a negative group is a free row); two clusters
//            are forbidden to each other when any row of one is forbidden to any row of the other
//   merges   distances, the Lance-Williams update, slot handling, tie rules and Z's layout and numbering are those above; each step merges the
//            ALLOWED live pair of least centroid distance (ties: lowest row slot, then lowest neighbour); the problem ends when no allowed pair
//            is left or when that least distance exceeds stop
//   output   merges[g] = the merges made; rows merges[g] .. of the problem's Z are zero.  No forbidden pair and stop = +inf: Z is
//            sdk_centroid_linkage's bit for bit.  stop = t: merges = cluster.cut_level of the stop = +inf run and the rows before it are the
//            same (every step is a global minimum over the allowed pairs, so fcluster_distance's argument carries over)
//   method   ahc_dist_kernel<true> stores +inf for a forbidden pair AFTER it has judged the computed distance (status 1 is decided on the
//            unmasked value; the diagonal is never masked, so a NaN / Inf row still shows itself).  centroid_lw then carries the constraint:
//            n_x inf^2 + .. - finite = +inf, and d_xy of a merged pair is finite, so no inf - inf arises; no scan ever picks +inf (every
//            comparison is a strict < against a running minimum that starts at +inf), so a row without an allowed neighbour holds
//            (nnd = +inf, nn = -1) and the pair search returning no row is the normal end.  A stale finite bound towards a pair that became
//            forbidden is caught by the lazy check D[x][y] == bound and rescanned like any other stale bound.
//
// Every index into D is int64 (a batch's distance storage passes 2^31 elements long before HBM runs out).  This file is compiled with
// -ffp-contract=off (Makefile): the update must round exactly as scipy's _centroid does.
#include <math.h>
#include <string.h>

#include "common.hpp"

namespace {

constexpr int TILE = 64;          // dist tile edge
constexpr int KC = 32;            // dims per LDS chunk
constexpr int MERGE_THREADS = 512;
constexpr int MERGE_WAVES = MERGE_THREADS / 64;
constexpr int TABLE_CHUNK = 64;   // problems per ahc_table_kernel launch (kernel-argument size)
constexpr int U = 8;              // independent loads in flight per thread in every sweep (the merge loop is latency-bound: one workgroup)

struct AhcProb {
  int64_t row0;    // first row of E
  int64_t n;       // rows
  int64_t off;     // byte offset of the problem's region in the workspace
  int64_t tile0;   // first dist tile of the problem (prefix over problems)
  int64_t zrow;    // first Z row (offsets[g] - g)
  int64_t pad;
};
struct AhcTableArgs {
  int count;
  int first;
  AhcProb p[TABLE_CHUNK];
};

// per-problem region: D [n][n] f64 | nnd [n] f64 | nn [n] i32 | sz [n] i32 | id [n] i32
__host__ __device__ inline int64_t r256(int64_t b) { return (b + 255) & ~(int64_t)255; }
__host__ __device__ inline int64_t tiles_of(int64_t n) { const int64_t t = (n + TILE - 1) / TILE; return t * (t + 1) / 2; }

struct Region {
  double* D; double* nnd; int32_t* nn; int32_t* sz; int32_t* id;
};
__device__ inline Region region(char* ws, const AhcProb& p) {
  char* b = ws + p.off;
  const int64_t n = p.n;
  Region r;
  r.D = (double*)b; b += r256(n * n * 8);
  r.nnd = (double*)b; b += r256(n * 8);
  r.nn = (int32_t*)b; b += r256(n * 4);
  r.sz = (int32_t*)b; b += r256(n * 4);
  r.id = (int32_t*)b;
  return r;
}

// the host's side of region(): the same five arrays in the same order -> the region's byte offset in the workspace
inline int64_t region_carve(WsCarver& c, int64_t n) {
  const int64_t off = (int64_t)c.bytes();
  c.take<double>((size_t)(n * n));
  c.take<double>((size_t)n);
  for (int i = 0; i < 3; ++i) c.take<int32_t>((size_t)n);
  return off;
}

__global__ void ahc_table_kernel(AhcProb* tab, AhcTableArgs a) {
  const int i = threadIdx.x;
  if (i < a.count) tab[a.first + i] = a.p[i];
}

// the problem whose [key(g), key(g + 1)) holds v: last g with key(g) <= v
template <typename F>
__device__ inline int find_prob(int G, int64_t v, F key) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (key(mid) <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <bool LINK>
__global__ void __launch_bounds__(256) ahc_dist_kernel(const float* __restrict__ E, int64_t ldE, int dim, const AhcProb* __restrict__ tab, int G,
                                                       char* ws, int32_t* status, const int32_t* __restrict__ group) {
  __shared__ double sm[2][TILE][KC + 1];       // the two row blocks of a k-chunk; afterwards the mirrored [64][65] output tile
  double (*sa)[KC + 1] = sm[0];
  double (*sb)[KC + 1] = sm[1];
  const int64_t bid = blockIdx.x;
  const int g = find_prob(G, bid, [&](int k) { return tab[k].tile0; });
  const AhcProb p = tab[g];
  const int64_t n = p.n;
  // linear tile index -> (ti, tj), ti <= tj, row-major over the upper triangle of nt x nt tiles
  const int64_t nt = (n + TILE - 1) / TILE;
  int64_t l = bid - p.tile0, ti = 0;
  {
    // rows before ti hold ti * nt - ti (ti - 1) / 2 tiles; solve, then fix up the float estimate
    const double b = 2.0 * nt + 1.0;
    ti = (int64_t)((b - sqrt(b * b - 8.0 * (double)l)) * 0.5);
    if (ti < 0) ti = 0;
    if (ti > nt - 1) ti = nt - 1;
    auto start = [&](int64_t r) { return r * nt - r * (r - 1) / 2; };
    while (ti > 0 && start(ti) > l) --ti;
    while (ti + 1 < nt && start(ti + 1) <= l) ++ti;
    l -= start(ti);
  }
  const int64_t tj = ti + l;
  const int64_t i0 = ti * TILE, j0 = tj * TILE;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  const float* Ea = E + (p.row0 + i0) * ldE;
  const float* Eb = E + (p.row0 + j0) * ldE;
  for (int k0 = 0; k0 < dim; k0 += KC) {
    for (int e = threadIdx.x; e < TILE * KC; e += 256) {
      const int r = e / KC, c = e % KC;
      const bool kin = k0 + c < dim;
      sa[r][c] = (kin && i0 + r < n) ? (double)Ea[(int64_t)r * ldE + k0 + c] : 0.0;
      sb[r][c] = (kin && j0 + r < n) ? (double)Eb[(int64_t)r * ldE + k0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < KC; ++c) {
      double va[4], vb[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) va[a] = sa[ty + 16 * a][c];
#pragma unroll
      for (int b = 0; b < 4; ++b) vb[b] = sb[tx + 16 * b][c];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double d = va[a] - vb[b];
          acc[a][b] = fma(d, d, acc[a][b]);
        }
    }
    __syncthreads();
  }
  Region R = region(ws, p);
  bool bad = false;
  int gi[4], gj[4];                             // LINK: the groups of this thread's rows and columns (-1: free, also past the end)
  if constexpr (LINK) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * a;
      gi[a] = i < n ? group[p.row0 + i] : -1;
      gj[a] = j < n ? group[p.row0 + j] : -1;
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      double v = sqrt(acc[a][b]);
      const bool in = i < n && j < n;
      if (in) bad |= !isfinite(v);              // judged before any masking
      if constexpr (LINK) {
        if (i != j && gi[a] >= 0 && gi[a] == gj[b]) v = INFINITY;
      }
      acc[a][b] = v;
      if (in) R.D[i * n + j] = v;
    }
  if (bad) status[g] = 1;
  if (ti == tj) return;                         // a diagonal tile wrote both triangles
  // the mirrored tile D[j][i], through LDS so the stores run along rows (sa / sb reused as one [64][65] double tile)
  double* tr = &sm[0][0][0];                    // 64 * 65 doubles fit in 2 * 64 * 33
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) tr[(tx + 16 * b) * 65 + ty + 16 * a] = acc[a][b];
  __syncthreads();
  for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
    const int r = e / TILE, c = e % TILE;
    const int64_t j = j0 + r, i = i0 + c;
    if (j < n && i < n) R.D[j * n + i] = tr[r * 65 + c];
  }
}

// (value, index) minimum with ties -> lower index
__device__ inline void take_min(double& v, int& i, double v2, int i2) {
  if (v2 < v || (v2 == v && i2 >= 0 && (i < 0 || i2 < i))) { v = v2; i = i2; }
}
__device__ inline void wave_min(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    take_min(v, i, v2, i2);
  }
}

__global__ void __launch_bounds__(256) ahc_nn_kernel(const AhcProb* __restrict__ tab, int G, int64_t n_total, char* ws) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_total) return;
  const int g = find_prob(G, row, [&](int k) { return tab[k].row0; });
  const AhcProb p = tab[g];
  Region R = region(ws, p);
  const int64_t r = row - p.row0;
  const int64_t n = p.n;
  const double* drow = R.D + r * n;
  double bv = INFINITY;
  int bi = -1;
  for (int64_t j0 = r + 1 + lane; j0 < n; j0 += 64 * U) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = j0 + 64 * u < n ? drow[j0 + 64 * u] : INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (v[u] < bv) { bv = v[u]; bi = (int)(j0 + 64 * u); }
  }
  wave_min(bv, bi);
  if (lane == 0) { R.nnd[r] = bv; R.nn[r] = bi; }
}

// scipy's _centroid, operation for operation; the max(0, .) is ours (scipy can take the square root of a small negative number -> NaN)
__device__ inline double centroid_lw(double dxz, double dyz, double dxy, int nx, int ny, int nz) {
  (void)nz;
  const double t = (((double)nx * dxz * dxz) + ((double)ny * dyz * dyz)) - ((double)((int64_t)nx * ny) * dxy * dxy) / (double)(nx + ny);
  return sqrt(fmax(0.0, t / (double)(nx + ny)));
}

template <bool LINK>
__global__ void __launch_bounds__(MERGE_THREADS) ahc_merge_kernel(const AhcProb* __restrict__ tab, int lds_rows, char* ws, double* Z, int32_t* status,
                                                                  double stop, int32_t* merges) {
  extern __shared__ __align__(16) char lds[];
  __shared__ double red_v[3][MERGE_WAVES];      // [0]: the pair search; [1], [2]: the rescans, alternating
  __shared__ int red_i[3][MERGE_WAVES];
  const int g = blockIdx.x;
  const AhcProb p = tab[g];
  const int64_t n = p.n;
  if (status[g] != 0 || n < 2) return;
  Region R = region(ws, p);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the per-row state in LDS when it fits (flat pointers: the same code reads either)
  double* nnd = R.nnd;
  int32_t* nn = R.nn;
  int32_t* sz = R.sz;
  if (n <= lds_rows) {
    nnd = (double*)lds;
    nn = (int32_t*)(lds + (size_t)lds_rows * 8);
    sz = (int32_t*)(lds + (size_t)lds_rows * 12);
    for (int64_t i = tid; i < n; i += MERGE_THREADS) { nnd[i] = R.nnd[i]; nn[i] = R.nn[i]; }
  }
  for (int64_t i = tid; i < n; i += MERGE_THREADS) { sz[i] = 1; R.id[i] = (int32_t)i; }
  double* D = R.D;
  double* Zg = Z + p.zrow * 4;
  __syncthreads();
  // LINK: the problem ends after t merges (uniform): the rest of its Z is zero
  auto finish = [&](int64_t t) {
    for (int64_t e = t * 4 + tid; e < (n - 1) * 4; e += MERGE_THREADS) Zg[e] = 0.0;
    if (tid == 0) merges[g] = (int32_t)t;
  };

  // nearest live j > r of row r (ties -> lowest j), skipping slot `dead`, by the whole workgroup; thread 0 stores it after a barrier.  The
  // partial slots alternate (1, 2) between calls: the next call may write while a slow thread still reads this one's.
  int rs = 0;
  auto rescan = [&](int64_t r, int64_t dead) {
    const double* row = D + r * n;
    double rv = INFINITY;
    int ri = -1;
    for (int64_t j0 = r + 1 + tid; j0 < n; j0 += MERGE_THREADS * U) {
      int lv[U];
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + MERGE_THREADS * u;
        lv[u] = (j < n && j != dead) ? sz[j] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = lv[u] > 0 ? row[j0 + MERGE_THREADS * u] : INFINITY;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (v[u] < rv) { rv = v[u]; ri = (int)(j0 + MERGE_THREADS * u); }
    }
    wave_min(rv, ri);
    const int b = 1 + (rs++ & 1);
    if (lane == 0) { red_v[b][wave] = rv; red_i[b][wave] = ri; }
    __syncthreads();
    if (tid == 0) {
      rv = red_v[b][0]; ri = red_i[b][0];
      for (int w = 1; w < MERGE_WAVES; ++w) take_min(rv, ri, red_v[b][w], red_i[b][w]);
      nnd[r] = rv; nn[r] = ri;
    }
  };

  for (int64_t t = 0; t < n - 1; ++t) {
    // A: the closest pair.  nnd[i] is a LOWER BOUND of row i's distance to its nearest live j > i (exact where it was last computed or
    // lowered; dead rows and rows with no live j > i hold +inf).  The row with the least bound (ties -> lowest row) is checked against its
    // stored neighbour: equal, and it is the global minimum; stale, and that row is rescanned and the search repeats.
    int64_t x = -1, y = -1;
    double dxy = 0.0;
    for (int64_t tries = 0;; ++tries) {
      double bv = INFINITY;
      int bi = -1;
      for (int64_t i0 = tid; i0 < n; i0 += MERGE_THREADS * U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = i0 + MERGE_THREADS * u < n ? nnd[i0 + MERGE_THREADS * u] : INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (v[u] < bv) { bv = v[u]; bi = (int)(i0 + MERGE_THREADS * u); }
      }
      wave_min(bv, bi);
      if (lane == 0) { red_v[0][wave] = bv; red_i[0][wave] = bi; }
      __syncthreads();
      bv = red_v[0][0]; bi = red_i[0][0];
      for (int w = 1; w < MERGE_WAVES; ++w) take_min(bv, bi, red_v[0][w], red_i[0][w]);
      if constexpr (LINK) {
        if (bi < 0) {                           // no allowed pair left: the normal end
          finish(t);
          return;
        }
      }
      if (bi < 0 || tries > n) {                // no finite pair left (non-finite distances); a bound is never rescanned twice per merge
        if (tid == 0) status[g] = 2;
        return;
      }
      x = bi; y = nn[x]; dxy = bv;
      if (y >= 0 && D[x * n + y] == bv) break;  // uniform: every thread read the same values after the barrier (y < 0: neighbour unknown)
      rescan(x, -1);
      __syncthreads();
    }
    if constexpr (LINK) {
      if (dxy > stop) {                         // the accepted minimum is exact: every allowed pair is above stop
        finish(t);
        return;
      }
    }
    const int nx = sz[x], ny = sz[y];
    // B + C: emit, Lance-Williams update of row / column y, bound upkeep of the rows below y (a smaller new distance, or an equal one when
    // y is below the stored neighbour, lowers the bound; else a row that pointed at x keeps its bound without a neighbour: any live slot
    // may sit at that bound, so only a rescan names the lowest).  sz / nnd / nn of slots x and y are read by every thread
    // above, so they change only after the next barrier (the loop below skips x and y itself)
    if (tid == 0) {
      const int ia = R.id[x], ib = R.id[y];
      Zg[t * 4 + 0] = (double)(ia < ib ? ia : ib);
      Zg[t * 4 + 1] = (double)(ia < ib ? ib : ia);
      Zg[t * 4 + 2] = dxy;
      Zg[t * 4 + 3] = (double)(nx + ny);
      R.id[y] = (int32_t)(n + t);
    }
    const double* Dx = D + x * n;
    double* Dy = D + y * n;
    for (int64_t z0 = tid; z0 < n; z0 += MERGE_THREADS * U) {
      int nz[U], c[U];
      double cur[U], ax[U], ay[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t z = z0 + MERGE_THREADS * u;
        const bool in = z < n;
        nz[u] = in ? sz[z] : 0;
        c[u] = in ? nn[z] : -1;
        cur[u] = in ? nnd[z] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t z = z0 + MERGE_THREADS * u;
        if (z == x || z == y) nz[u] = 0;
        ax[u] = nz[u] ? Dx[z] : 0.0;
        ay[u] = nz[u] ? Dy[z] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!nz[u]) continue;
        const int64_t z = z0 + MERGE_THREADS * u;
        const double v = centroid_lw(ax[u], ay[u], dxy, nx, ny, nz[u]);
        Dy[z] = v;
        D[z * n + y] = v;
        if (z < y) {
          if (v < cur[u] || (v == cur[u] && (int)y < c[u])) { nnd[z] = v; nn[z] = (int32_t)y; }
          else if (c[u] == (int)x) nn[z] = -1;
        }
      }
    }
    __syncthreads();
    // D: slot x dies, slot y holds the merged cluster (the rescan skips x by index and only tests sz[j] > 0, so these stores need no barrier
    // of their own); row y's nearest neighbour is recomputed exactly
    if (tid == 0) { sz[x] = 0; sz[y] = nx + ny; nnd[x] = INFINITY; nn[x] = -1; }
    rescan(y, x);
    __syncthreads();
  }
  if constexpr (LINK) finish(n - 1);
}

size_t ahc_workspace_bytes(const int32_t* offsets, int G) {
  WsCarver c{};
  c.take<AhcProb>((size_t)G);                          // the table lives at the start of the workspace
  for (int g = 0; g < G; ++g) region_carve(c, (int64_t)offsets[g + 1] - offsets[g]);
  return c.bytes();
}

// group == nullptr: sdk_centroid_linkage (stop and merges unused); else sdk_linked_linkage
int launch_all(const char* fn, sdk_ctx* ctx, const float* E, int ldE, int dim, const int32_t* group, const int32_t* offsets, int G, double stop, double* Z,
               int32_t* merges, int32_t* status, void* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  WsCarver carve{(char*)ws, 0};
  AhcProb* tab = carve.take<AhcProb>((size_t)G);
  int64_t tiles = 0;
  for (int g = 0; g < G; ++g) tiles += tiles_of((int64_t)offsets[g + 1] - offsets[g]);
  SDK_REQUIRE(tiles < (int64_t)INT32_MAX, "%s: %lld distance tiles exceed one launch", fn, (long long)tiles);
  int64_t max_n = 0;
  tiles = 0;
  AhcTableArgs a;
  memset(&a, 0, sizeof(a));
  for (int g0 = 0; g0 < G; g0 += TABLE_CHUNK) {
    a.first = g0;
    a.count = G - g0 < TABLE_CHUNK ? G - g0 : TABLE_CHUNK;
    for (int i = 0; i < a.count; ++i) {
      const int g = g0 + i;
      const int64_t n = (int64_t)offsets[g + 1] - offsets[g];
      a.p[i] = AhcProb{offsets[g], n, region_carve(carve, n), tiles, (int64_t)offsets[g] - g, 0};
      tiles += tiles_of(n);
      max_n = n > max_n ? n : max_n;
    }
    hipLaunchKernelGGL(ahc_table_kernel, dim3(1), dim3(TABLE_CHUNK), 0, s, tab, a);
    SDK_LAUNCH_CHECK();
  }
  const int64_t n_total = (int64_t)offsets[G] - offsets[0];
  SDK_HIP_OK(hipMemsetAsync(status, 0, (size_t)G * 4, s));
  if (group) {
    SDK_HIP_OK(hipMemsetAsync(merges, 0, (size_t)G * 4, s));
    hipLaunchKernelGGL(ahc_dist_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, s, E, (int64_t)ldE, dim, (const AhcProb*)tab, G, (char*)ws, status, group);
  } else {
    hipLaunchKernelGGL(ahc_dist_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, s, E, (int64_t)ldE, dim, (const AhcProb*)tab, G, (char*)ws, status, group);
  }
  SDK_LAUNCH_CHECK();
  hipLaunchKernelGGL(ahc_nn_kernel, dim3((unsigned)((n_total + 3) / 4)), dim3(256), 0, s, (const AhcProb*)tab, G, n_total, (char*)ws);
  SDK_LAUNCH_CHECK();
  if (ctx->ahc_distances_only) return 0;
  // per-row state in LDS up to 8192 rows (16 B per row: nnd, nn, sz); larger problems keep it in the workspace
  const int lds_rows = (int)(max_n < 8192 ? max_n : 8192);
  const int lds = lds_rows * 16;
  if (group) {
    if (lds > 64 * 1024 && sdk_lds_optin(ctx, (const void*)ahc_merge_kernel<true>, 8192 * 16)) return 1;
    hipLaunchKernelGGL(ahc_merge_kernel<true>, dim3(G), dim3(MERGE_THREADS), lds, s, (const AhcProb*)tab, lds_rows, (char*)ws, Z, status, stop, merges);
  } else {
    if (lds > 64 * 1024 && sdk_lds_optin(ctx, (const void*)ahc_merge_kernel<false>, 8192 * 16)) return 1;
    hipLaunchKernelGGL(ahc_merge_kernel<false>, dim3(G), dim3(MERGE_THREADS), lds, s, (const AhcProb*)tab, lds_rows, (char*)ws, Z, status, stop, merges);
  }
  SDK_LAUNCH_CHECK();
  return 0;
}

constexpr int AHC_MAX_N = 65536;    // the condensed distance count of one problem stays under 2^31
constexpr int AHC_MAX_DIM = 2048;
// the host-side refusals shared by both entry points: 0 = the offsets describe G problems the kernels serve
int check_ahc_offsets(const char* fn, const int32_t* offsets, int G, int dim) {
  SDK_REQUIRE(offsets, "%s: offsets is null", fn);
  SDK_REQUIRE(G >= 1, "%s: G=%d (at least one problem)", fn, G);
  SDK_REQUIRE(dim >= 1 && dim <= AHC_MAX_DIM, "%s: dim=%d (served: 1 .. %d)", fn, dim, AHC_MAX_DIM);
  SDK_REQUIRE(offsets[0] == 0, "%s: offsets[0]=%d (the first problem starts at row 0)", fn, offsets[0]);
  for (int g = 0; g < G; ++g) {
    const int64_t n = (int64_t)offsets[g + 1] - offsets[g];
    SDK_REQUIRE(n >= 1, "%s: offsets not increasing at problem %d (offsets[%d]=%d, offsets[%d]=%d: every problem needs a row)", fn, g, g, offsets[g],
                g + 1, offsets[g + 1]);
    SDK_REQUIRE(n <= AHC_MAX_N, "%s: problem %d has n=%lld rows (at most %d)", fn, g, (long long)n, AHC_MAX_N);
  }
  return 0;
}
}  // namespace

// ---- the entry points: host-side comparisons only (no floating-point arithmetic for -ffp-contract to bear on), then launch_all
extern "C" size_t sdk_centroid_linkage_workspace_bytes(const int32_t* offsets, int G, int dim) {
  if (check_ahc_offsets("sdk_centroid_linkage_workspace_bytes", offsets, G, dim)) return 0;
  return ahc_workspace_bytes(offsets, G);
}

extern "C" int sdk_centroid_linkage(sdk_ctx* ctx, const float* E, int ldE, int dim, const int32_t* offsets, int G, double* Z, int32_t* status,
                                    void* workspace, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx && E && Z && status && workspace, "sdk_centroid_linkage: null argument (ctx=%p E=%p Z=%p status=%p workspace=%p)", (void*)ctx,
              (const void*)E, (void*)Z, (void*)status, workspace);
  if (int rc = check_ahc_offsets("sdk_centroid_linkage", offsets, G, dim)) return rc;
  SDK_REQUIRE(ldE >= dim, "sdk_centroid_linkage: ldE=%d < dim=%d", ldE, dim);
  SDK_REQUIRE((uintptr_t)E % 4 == 0 && (uintptr_t)Z % 8 == 0 && (uintptr_t)status % 4 == 0 && (uintptr_t)workspace % 256 == 0,
              "sdk_centroid_linkage: misaligned pointer (E=%p needs 4, Z=%p needs 8, status=%p needs 4, workspace=%p needs 256 bytes)",
              (const void*)E, (void*)Z, (void*)status, workspace);
  SDK_REQUIRE_WS("sdk_centroid_linkage", "sdk_centroid_linkage_workspace_bytes", workspace, ws_bytes, ahc_workspace_bytes(offsets, G), 1);
  return launch_all("sdk_centroid_linkage", ctx, E, ldE, dim, nullptr, offsets, G, 0.0, Z, nullptr, status, workspace, stream);
}

extern "C" size_t sdk_linked_linkage_workspace_bytes(const int32_t* offsets, int G, int dim) {
  if (check_ahc_offsets("sdk_linked_linkage_workspace_bytes", offsets, G, dim)) return 0;
  return ahc_workspace_bytes(offsets, G);
}

extern "C" int sdk_linked_linkage(sdk_ctx* ctx, const float* E, int ldE, int dim, const int32_t* group, const int32_t* offsets, int G, double stop,
                                  double* Z, int32_t* merges, int32_t* status, void* workspace, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx && E && group && Z && merges && status && workspace,
              "sdk_linked_linkage: null argument (ctx=%p E=%p group=%p Z=%p merges=%p status=%p workspace=%p)", (void*)ctx, (const void*)E,
              (const void*)group, (void*)Z, (void*)merges, (void*)status, workspace);
  if (int rc = check_ahc_offsets("sdk_linked_linkage", offsets, G, dim)) return rc;
  SDK_REQUIRE(ldE >= dim, "sdk_linked_linkage: ldE=%d < dim=%d", ldE, dim);
  SDK_REQUIRE(stop >= 0.0, "sdk_linked_linkage: stop=%g (a distance >= 0, or +inf for every allowed merge)", stop);     // false for a NaN too
  SDK_REQUIRE((uintptr_t)E % 4 == 0 && (uintptr_t)group % 4 == 0 && (uintptr_t)Z % 8 == 0 && (uintptr_t)merges % 4 == 0 && (uintptr_t)status % 4 == 0 &&
                  (uintptr_t)workspace % 256 == 0,
              "sdk_linked_linkage: misaligned pointer (E=%p needs 4, group=%p needs 4, Z=%p needs 8, merges=%p needs 4, status=%p needs 4, workspace=%p "
              "needs 256 bytes)", (const void*)E, (const void*)group, (void*)Z, (void*)merges, (void*)status, workspace);
  SDK_REQUIRE_WS("sdk_linked_linkage", "sdk_linked_linkage_workspace_bytes", workspace, ws_bytes, ahc_workspace_bytes(offsets, G), 1);
  return launch_all("sdk_linked_linkage", ctx, E, ldE, dim, group, offsets, G, stop, Z, merges, status, workspace, stream);
}
