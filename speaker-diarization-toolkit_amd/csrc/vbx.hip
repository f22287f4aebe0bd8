// VBx clustering (plda.py, cluster.vbx_cluster): the PLDA transform of the training embeddings, the variational-Bayes mixture that re-estimates
// the speakers the centroid linkage initialised, and the responsibility-weighted centroids the assignment stage reads.  Float64 throughout.
//
//   plda_transform_kernel   E rows -> X [n][D]: the front transform of plda_front.hpp (centre, length-normalise, LDA, centre, length-normalise),
//                           then the PLDA basis.  Block = 4 rows, thread = a column; every dot product runs over its index in ascending order.
//   vbx_reset_kernel        pi = 1 / S, elbo = 0, n_iter = status = done = 0
//   vbx_init_kernel         wave = one row: rho = x sqrt(Phi), G_t, gamma0 from the initial labels; a non-finite rho sets status and done
//   vbx_stats_kernel        block = (64-row block b, 16 speakers): partial N[b][s] and F[b][s][:] = sum over the block's rows, ascending; and the
//                           block's partial of sum_t lse_t
//   vbx_finish_kernel       one block: N_s = partials in block order; ELBO, the stop test, n_iter and pi
//   vbx_mstep_kernel        block = speaker: F_s = partials in block order, invL, alpha, and the two per-speaker sums over d (block_sum, reduce.hpp)
//   vbx_estep_kernel        wave = 4 rows at a time, lane = speaker (lane-strided over any S): z, lse, gamma
//   vbx_keep_kernel / vbx_labels_kernel / vbx_centroids_kernel   speakers with pi > 1e-7, the rows' hard labels, the kept speakers' centroids
//   vbx_chain_kernel / vbx_chain_mem_kernel / vbx_hmm_post_kernel / vbx_hmm_finish_kernel   sdk_vbx_hmm: the HMM's forward and backward passes over
//                           rows in time order, gamma and pi' (described where they stand)
//
// Every sum over rows runs over fixed 64-row blocks whose partials are combined in block order (the centroids: one pass in ascending row
// order); no floating-point atomics; one owner per output element: results are bit-identical run to run.  The iterations are enqueued back to
// back; the stop test runs on the device (vbx_finish_kernel sets `done`), and every later launch leaves at its first instruction.
#include "common.hpp"
#include "plda_front.hpp"

#include <math.h>

namespace {

constexpr int VB_NT = 256;
constexpr int VB_ROWS = 64;          // rows per block of every sum over rows
constexpr int VB_SC = 16;            // speakers per block of the statistics kernel
constexpr int VB_MAX_ROWS = 65536;   // diarize.MAX_LINKAGE_ROWS
constexpr int VB_ST_NONFINITE = 1, VB_ST_LABEL = 2, VB_ST_ELBO = 4;

__global__ __launch_bounds__(PLDA_NT) void plda_transform_kernel(const float* __restrict__ E, int d_in, const int32_t* __restrict__ rows, int n,
                                                                 const double* __restrict__ mean1, const double* __restrict__ lda,
                                                                 const double* __restrict__ mean2, const double* __restrict__ mu,
                                                                 const double* __restrict__ Tt, int D0, int D, double* __restrict__ X) {
  __shared__ double s_a[PLDA_RPB][PLDA_MAX_DIM];
  __shared__ double s_b[PLDA_RPB][PLDA_MAX_DIM];
  __shared__ double s_red[PLDA_NT / 64];
  const int tid = threadIdx.x, i0 = blockIdx.x * PLDA_RPB;
  // 1, 2: x2 (plda_front.hpp), stored minus mu
  plda_front([&](int r) { return i0 + r < n ? E + (int64_t)rows[i0 + r] * d_in : nullptr; }, d_in, mean1, lda, mean2, D0, s_a, s_red,
             [&](int r, int j, double x2) { s_b[r][j] = x2 - mu[j]; });
  __syncthreads();
  // 3: x = ((x2 - mu) T^T)[:D]; Tt [D0][D] holds the first D rows of T, transposed
  for (int j = tid; j < D; j += PLDA_NT) {
    double acc[PLDA_RPB];
#pragma unroll
    for (int r = 0; r < PLDA_RPB; ++r) acc[r] = 0.0;
    for (int k = 0; k < D0; ++k) {
      const double t = Tt[(int64_t)k * D + j];
#pragma unroll
      for (int r = 0; r < PLDA_RPB; ++r) acc[r] = fma(s_b[r][k], t, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < PLDA_RPB; ++r)
      if (i0 + r < n) X[(int64_t)(i0 + r) * D + j] = acc[r];
  }
}

// the device-side state of one sdk_vbx call, carved from its workspace
struct VbxWs {
  double *rho, *G, *lse, *Npart, *Fpart, *lsepart, *N, *alphaT, *cs, *es, *prev;
  int32_t* done;
};

__global__ __launch_bounds__(64) void vbx_reset_kernel(int S, int max_iters, double* __restrict__ pi, double* __restrict__ elbo,
                                                       int32_t* __restrict__ n_iter, int32_t* __restrict__ status, VbxWs w) {
  const int tid = threadIdx.x;
  for (int s = tid; s < S; s += 64) pi[s] = 1.0 / (double)S;
  for (int i = tid; i < max_iters; i += 64) elbo[i] = 0.0;
  if (tid == 0) {
    *n_iter = 0;
    *status = 0;
    *w.done = 0;
    *w.prev = 0.0;
  }
}

// wave = one row
__global__ __launch_bounds__(VB_NT) void vbx_init_kernel(const double* __restrict__ X, const double* __restrict__ Phi,
                                                         const int32_t* __restrict__ labels, int n, int D, int S, double init_smoothing,
                                                         double* __restrict__ gamma, int32_t* __restrict__ status, VbxWs w) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (VB_NT / 64) + (threadIdx.x >> 6);
  if (t >= n) return;
  double q = 0.0;
  bool bad = false;
  for (int d = lane; d < D; d += 64) {
    const double x = X[(int64_t)t * D + d];
    const double r = x * sqrt(Phi[d]);
    w.rho[(int64_t)t * D + d] = r;
    q = fma(x, x, q);
    bad = bad || !isfinite(r);
  }
  q = wave_sum(q);
  const int lab = labels[t];
  if (lane == 0) w.G[t] = -0.5 * (q + (double)D * 1.8378770664093454835606594728112);      // ln 2 pi
  if (bad) { atomicOr(status, VB_ST_NONFINITE); *w.done = 1; }
  if (lane == 0 && (unsigned)lab >= (unsigned)S) { atomicOr(status, VB_ST_LABEL); *w.done = 1; }
  const double off = exp(-init_smoothing);                               // softmax with the maximum subtracted
  const double den = 1.0 + (double)(S - 1) * off;
  for (int s = lane; s < S; s += 64) gamma[(int64_t)t * S + s] = (s == lab ? 1.0 : off) / den;
}

// grid (row blocks, speaker chunks), block = D threads: thread d owns column d of the chunk's F partials
__global__ __launch_bounds__(128) void vbx_stats_kernel(const double* __restrict__ gamma, int n, int D, int S, int with_lse, VbxWs w) {
  if (*w.done) return;
  const int b = blockIdx.x, s0 = blockIdx.y * VB_SC, d = threadIdx.x;
  const int t0 = b * VB_ROWS, m = min(VB_ROWS, n - t0), ns = min(VB_SC, S - s0);
  double acc[VB_SC];
#pragma unroll
  for (int k = 0; k < VB_SC; ++k) acc[k] = 0.0;
  for (int i = 0; i < m; ++i) {
    const double r = w.rho[(int64_t)(t0 + i) * D + d];
    const double* g = gamma + (int64_t)(t0 + i) * S + s0;
#pragma unroll
    for (int k = 0; k < VB_SC; ++k)
      if (k < ns) acc[k] = fma(g[k], r, acc[k]);
  }
#pragma unroll
  for (int k = 0; k < VB_SC; ++k)
    if (k < ns) w.Fpart[((int64_t)b * S + s0 + k) * D + d] = acc[k];
  if (d < ns) {
    double a = 0.0;
    for (int i = 0; i < m; ++i) a += gamma[(int64_t)(t0 + i) * S + s0 + d];
    w.Npart[(int64_t)b * S + s0 + d] = a;
  }
  if (with_lse && blockIdx.y == 0 && d < 64) {                           // the first wave (D is 64 or 128)
    const double v = wave_sum(d < m ? w.lse[t0 + d] : 0.0);
    if (d == 0) w.lsepart[b] = v;
  }
}

// one block.  ii < 0: the speakers' N only (before the first iteration)
__global__ __launch_bounds__(VB_NT) void vbx_finish_kernel(int nblk, int S, int ii, double epsilon, double* __restrict__ pi,
                                                           double* __restrict__ elbo, int32_t* __restrict__ n_iter, int32_t* __restrict__ status,
                                                           VbxWs w) {
  __shared__ double s_tot;
  if (*w.done) return;
  const int tid = threadIdx.x;
  for (int s = tid; s < S; s += VB_NT) {
    double a = 0.0;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) a += w.Npart[(int64_t)b * S + s];
    w.N[s] = a;
  }
  if (ii < 0) return;
  __syncthreads();
  if (tid == 0) {
    double L = 0.0, e2 = 0.0, tot = 0.0;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) L += w.lsepart[b];
    for (int s = 0; s < S; ++s) e2 += w.es[s];
    for (int s = 0; s < S; ++s) tot += w.N[s];
    const double v = L + e2;
    elbo[ii] = v;
    *n_iter = ii + 1;
    s_tot = tot;
    const bool fin = isfinite(v);
    if (!fin) atomicOr(status, VB_ST_ELBO);
    if (!fin || (ii > 0 && v - *w.prev < epsilon)) *w.done = 1;
    *w.prev = v;
  }
  __syncthreads();
  for (int s = tid; s < S; s += VB_NT) pi[s] = w.N[s] / s_tot;
}

// block = speaker s, thread = dimension d
__global__ __launch_bounds__(128) void vbx_mstep_kernel(const double* __restrict__ Phi, int nblk, int D, int S, double Fa, double Fb, VbxWs w) {
  __shared__ double s_red[2];
  if (*w.done) return;
  const int s = blockIdx.x, d = threadIdx.x;
  double F = 0.0;
#pragma unroll 8
  for (int b = 0; b < nblk; ++b) F += w.Fpart[((int64_t)b * S + s) * D + d];
  const double fab = Fa / Fb, ph = Phi[d];
  const double invL = 1.0 / (1.0 + fab * w.N[s] * ph);
  const double al = fab * invL * F;
  w.alphaT[(int64_t)d * S + s] = al;
  const double c = block_sum((invL + al * al) * ph, s_red);
  const double e = block_sum(log(invL) - invL - al * al + 1.0, s_red);
  if (d == 0) {
    w.cs[s] = -0.5 * c;
    w.es[s] = 0.5 * Fb * e;
  }
}

// block = one 64-row block, wave = 16 of its rows, four at a time; lane = speaker, strided over any S.  z goes through the gamma buffer.
// LOGP (sdk_vbx_hmm): `gamma` is the logp buffer; logp[t][s] = z without ln pi is stored and the softmax is left out.  LOGP = false is sdk_vbx's
// kernel, instruction for instruction.
template <bool LOGP>
__global__ __launch_bounds__(VB_NT) void vbx_estep_kernel(const double* __restrict__ pi, int n, int D, int S, double Fa, double* __restrict__ gamma,
                                                          VbxWs w) {
  if (*w.done) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double ninf = -HUGE_VAL;
  for (int q = 0; q < 4; ++q) {
    const int ta = blockIdx.x * VB_ROWS + wave * 16 + q * 4;             // wave-uniform
    if (ta >= n) return;
    const int nr = min(4, n - ta);
    const double* rr[4];
    double M[4], G[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = ta + min(r, nr - 1);                                 // a row past the end repeats the last one and is not stored
      rr[r] = w.rho + (int64_t)t * D;
      G[r] = w.G[t];
      M[r] = ninf;
    }
    for (int s0 = 0; s0 < S; s0 += 64) {
      const int s = s0 + lane;
      const bool act = s < S;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      for (int d = 0; d < D; ++d) {
        const double a = act ? w.alphaT[(int64_t)d * S + s] : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = fma(rr[r][d], a, acc[r]);
      }
      if (act) {
        const double c = w.cs[s], lp = LOGP ? 0.0 : log(pi[s]);          // pi == 0: z = -inf, gamma exactly 0
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double z = LOGP ? Fa * (acc[r] + c + G[r]) : Fa * (acc[r] + c + G[r]) + lp;
          if (r < nr) gamma[(int64_t)(ta + r) * S + s] = z;
          M[r] = fmax(M[r], z);
        }
      }
    }
    if (LOGP) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) M[r] = wave_max(M[r]);
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = lane; s < S; s += 64) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < nr) sum[r] += exp(gamma[(int64_t)(ta + r) * S + s] - M[r]);
    }
    double lse[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lse[r] = M[r] + log(wave_sum(sum[r]));
    for (int s = lane; s < S; s += 64) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < nr) {
          double* g = gamma + (int64_t)(ta + r) * S + s;
          *g = exp(*g - lse[r]);
        }
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < nr) w.lse[ta + r] = lse[r];
    }
  }
}

__global__ __launch_bounds__(64) void vbx_keep_kernel(const double* __restrict__ pi, int S, int32_t* __restrict__ K, int32_t* __restrict__ keep) {
  if (threadIdx.x != 0) return;
  int k = 0;
  for (int s = 0; s < S; ++s)
    if (pi[s] > 1e-7) keep[k++] = s;                                     // a NaN is not kept
  *K = k;
  for (; k < S; ++k) keep[k] = -1;
}

__global__ __launch_bounds__(VB_NT) void vbx_labels_kernel(const double* __restrict__ gamma, int n, int S, const int32_t* __restrict__ K,
                                                           const int32_t* __restrict__ keep, int32_t* __restrict__ labels) {
  const int t = blockIdx.x * VB_NT + threadIdx.x;
  if (t >= n) return;
  const int Kn = *K;
  int best = -1;
  double bv = 0.0;
  for (int k = 0; k < Kn; ++k) {
    const double v = gamma[(int64_t)t * S + keep[k]];
    if (best < 0 || v > bv) { bv = v; best = k; }                        // ties to the lower speaker
  }
  labels[t] = best;
}

// block = kept speaker k, thread = the columns tid, tid + 256.  The rows pass through LDS in tiles with their responsibilities; every thread
// walks them in ascending order, so a column's float64 sum has one owner and one order.  Then the weighted mean, its norm, the unit row.
__global__ __launch_bounds__(VB_NT) void vbx_centroids_kernel(const double* __restrict__ gamma, const float* __restrict__ E,
                                                              const int32_t* __restrict__ rows, int n, int S, int d, const int32_t* __restrict__ K,
                                                              const int32_t* __restrict__ keep, float* __restrict__ cent, double* __restrict__ cent64) {
  __shared__ int32_t s_row[VB_NT];
  __shared__ double s_g[VB_NT];
  __shared__ double s_red[VB_NT / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= *K) return;                                                   // uniform over the block
  const int s = keep[k];
  const int j0 = tid, j1 = tid + VB_NT;
  const bool h0 = j0 < d, h1 = j1 < d;
  double a0 = 0.0, a1 = 0.0, wsum = 0.0;
  for (int i0 = 0; i0 < n; i0 += VB_NT) {
    const int m = min(VB_NT, n - i0);
    __syncthreads();
    if (tid < m) {
      s_row[tid] = rows[i0 + tid];
      s_g[tid] = gamma[(int64_t)(i0 + tid) * S + s];
    }
    __syncthreads();
#pragma unroll 8
    for (int i = 0; i < m; ++i) {
      const float* e = E + (int64_t)s_row[i] * d;
      const double g = s_g[i];
      wsum += g;
      if (h0) a0 = fma(g, (double)e[j0], a0);
      if (h1) a1 = fma(g, (double)e[j1], a1);
    }
  }
  if (wsum > 0.0) { a0 /= wsum; a1 /= wsum; }
  const double nrm = fmax(sqrt(block_sum((h0 ? a0 * a0 : 0.0) + (h1 ? a1 * a1 : 0.0), s_red)), 1e-300);
  a0 /= nrm;
  a1 /= nrm;
  if (h0) {
    cent[(int64_t)k * d + j0] = (float)a0;
    cent64[(int64_t)k * d + j0] = a0;
  }
  if (h1) {
    cent[(int64_t)k * d + j1] = (float)a1;
    cent64[(int64_t)k * d + j1] = a1;
  }
}

// ---- the HMM of sdk_vbx_hmm: logp [n][S] (vbx_estep_kernel<true>), the forward and backward chains, gamma and the partials of pi'
//
//   vbx_chain_kernel<K>     ONE launch of two blocks of one wave: block 0 the forward pass, block 1 the backward pass, side by side.  Lane l holds
//                           speakers l, l + 64, .. in K registers (S <= 64 K, K <= VH_MAXK: S <= 256); a step is two cross-lane reductions (the
//                           maximum, the sum of exponentials: DPP inside a row of 16 lanes, then the four rows through v_readlane), no barrier,
//                           no LDS and no load the recurrence waits for: the logp rows, which do not depend on it, are loaded VH_PF .. 2 VH_PF
//                           steps ahead into two register buffers.  lf, lb [n][S] and m [n] leave by plain vector stores.
//   vbx_chain_mem_kernel    the same passes for S > 256: a lane's speakers do not fit its registers, so it re-reads the previous row of lf / lb,
//                           of which it wrote every element it reads (no other lane's stores are read: no fence), three sweeps per step.
//   vbx_hmm_post_kernel     block = 64-row block, thread = speaker: gamma, and the block's partial of sum_{t >= 1} exp(m[t-1] + logp + lb - tll)
//                           in ascending row order
//   vbx_hmm_finish_kernel   one block: N_s and pi' from the partials in block order, the ELBO, the stop test, n_iter and pi
// Reduction orders: per lane over its registers ascending, then lanes l ^ 1, l ^ 2, l ^ 4, l ^ 8 (the xor butterfly), then rows (0 + 1) + (2 + 3).
struct VbxHmmWs {
  double *logp, *lf, *lb, *m, *pipart, *pinew;
};

constexpr int VH_PF = 4;             // logp rows per register buffer of the chain (two buffers: a row is loaded 4 .. 8 steps before its use; the
                                     // step is unrolled 2 VH_PF times per direction, and at K = 4 that is the instruction cache's 64 KB)
constexpr int VH_MAXK = 4;           // speakers per lane that the chain holds in registers: S <= 256

// the value of lane DPP(l) in every lane; CTRL permutes inside rows of 16 lanes, so every lane reads a live one
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false), __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false));
}

__device__ __forceinline__ double lane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// quad_perm [1,0,3,2] and [2,3,0,1] are l ^ 1 and l ^ 2; after them a quad is uniform, so row_half_mirror (l -> 7 - l) reads what l ^ 4 holds, and
// row_mirror (l -> 15 - l) what l ^ 8 holds.  Whole wave active, uniform control flow only.
__device__ __forceinline__ double chain_max(double v) {
  v = fmax(v, dpp_d<0xB1>(v));
  v = fmax(v, dpp_d<0x4E>(v));
  v = fmax(v, dpp_d<0x141>(v));
  v = fmax(v, dpp_d<0x140>(v));
  return fmax(fmax(lane_d(v, 0), lane_d(v, 16)), fmax(lane_d(v, 32), lane_d(v, 48)));
}

__device__ __forceinline__ double chain_sum(double v) {
  v += dpp_d<0xB1>(v);
  v += dpp_d<0x4E>(v);
  v += dpp_d<0x141>(v);
  v += dpp_d<0x140>(v);
  return (lane_d(v, 0) + lane_d(v, 16)) + (lane_d(v, 32) + lane_d(v, 48));
}

// ln(e^a + e^b) = max + log1p(exp(min - max)); -inf with a finite other argument returns that argument exactly; both -inf: -inf
__device__ __forceinline__ double logaddexp_d(double a, double b) {
  const double hi = fmax(a, b), lo = fmin(a, b);
  return hi == -HUGE_VAL ? hi : hi + log1p(exp(lo - hi));
}

// logsumexp over the wave's K registers per lane, the maximum subtracted
template <int K>
__device__ __forceinline__ double chain_lse(const double (&u)[K]) {
  double mx = u[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = fmax(mx, u[k]);
  mx = chain_max(mx);
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) sum += exp(u[k] - mx);
  return mx + log(chain_sum(sum));
}

// row min(max(t, 0), n - 1) of logp: lane's K speakers; 0 for a speaker past S (whose ln pi is -inf)
template <int K>
__device__ __forceinline__ void chain_load(const double* __restrict__ logp, int t, int n, int S, int lane, double (&dst)[K]) {
  const double* row = logp + (int64_t)min(max(t, 0), n - 1) * S;
#pragma unroll
  for (int k = 0; k < K; ++k) dst[k] = lane + 64 * k < S ? row[lane + 64 * k] : 0.0;
}

template <int K>
__global__ __launch_bounds__(64) void vbx_chain_kernel(const double* __restrict__ pi, int n, int S, double lnP, double ln1mP, VbxWs w, VbxHmmWs h) {
  if (*w.done) return;
  const int lane = threadIdx.x;
  const double* __restrict__ logp = h.logp;
  double lnpi[K], x[K], u[K], A[VH_PF][K], B[VH_PF][K];
#pragma unroll
  for (int k = 0; k < K; ++k) lnpi[k] = lane + 64 * k < S ? log(pi[lane + 64 * k]) : -HUGE_VAL;      // pi == 0: -inf
  if (blockIdx.x == 0) {
    // forward: x = lf[t - 1]
    double* __restrict__ lf = h.lf;
    double c[K];
    chain_load<K>(logp, 0, n, S, lane, u);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      c[k] = ln1mP + lnpi[k];
      x[k] = u[k] + lnpi[k];
      if (lane + 64 * k < S) lf[lane + 64 * k] = x[k];
    }
    auto step = [&](const double (&lp)[K], int t) {
      const double m = chain_lse<K>(x);
      if (lane == 0) h.m[t - 1] = m;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        x[k] = lp[k] + logaddexp_d(lnP + x[k], c[k] + m);
        if (lane + 64 * k < S) lf[(int64_t)t * S + lane + 64 * k] = x[k];
      }
    };
#pragma unroll
    for (int j = 0; j < VH_PF; ++j) chain_load<K>(logp, 1 + j, n, S, lane, A[j]);
    for (int t0 = 1; t0 < n; t0 += 2 * VH_PF) {                           // t0 and n are wave-uniform
#pragma unroll
      for (int j = 0; j < VH_PF; ++j) chain_load<K>(logp, t0 + VH_PF + j, n, S, lane, B[j]);
#pragma unroll
      for (int j = 0; j < VH_PF; ++j)
        if (t0 + j < n) step(A[j], t0 + j);
#pragma unroll
      for (int j = 0; j < VH_PF; ++j) chain_load<K>(logp, t0 + 2 * VH_PF + j, n, S, lane, A[j]);
#pragma unroll
      for (int j = 0; j < VH_PF; ++j)
        if (t0 + VH_PF + j < n) step(B[j], t0 + VH_PF + j);
    }
    const double m = chain_lse<K>(x);
    if (lane == 0) h.m[n - 1] = m;                                        // tll
  } else {
    // backward: x = lb[t + 1], lp = logp[t + 1]
    double* __restrict__ lb = h.lb;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      x[k] = 0.0;
      if (lane + 64 * k < S) lb[(int64_t)(n - 1) * S + lane + 64 * k] = 0.0;
    }
    auto step = [&](const double (&lp)[K], int t) {
      double q[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        q[k] = lp[k] + x[k];
        u[k] = lnpi[k] + q[k];
      }
      const double r = ln1mP + chain_lse<K>(u);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        x[k] = logaddexp_d(lnP + q[k], r);
        if (lane + 64 * k < S) lb[(int64_t)t * S + lane + 64 * k] = x[k];
      }
    };
#pragma unroll
    for (int j = 0; j < VH_PF; ++j) chain_load<K>(logp, n - 1 - j, n, S, lane, A[j]);
    for (int t0 = n - 2; t0 >= 0; t0 -= 2 * VH_PF) {                      // step j of a buffer: row t = t0 - j, reading logp[t + 1]
#pragma unroll
      for (int j = 0; j < VH_PF; ++j) chain_load<K>(logp, t0 - VH_PF - j + 1, n, S, lane, B[j]);
#pragma unroll
      for (int j = 0; j < VH_PF; ++j)
        if (t0 - j >= 0) step(A[j], t0 - j);
#pragma unroll
      for (int j = 0; j < VH_PF; ++j) chain_load<K>(logp, t0 - 2 * VH_PF - j + 1, n, S, lane, A[j]);
#pragma unroll
      for (int j = 0; j < VH_PF; ++j)
        if (t0 - VH_PF - j >= 0) step(B[j], t0 - VH_PF - j);
    }
  }
}

// S > 256.  lf and lb are read back by the lane that wrote them, through the pointer that wrote them.
__global__ __launch_bounds__(64) void vbx_chain_mem_kernel(const double* __restrict__ pi, int n, int S, double lnP, double ln1mP, VbxWs w, VbxHmmWs h) {
  if (*w.done) return;
  const int lane = threadIdx.x;
  const double* __restrict__ logp = h.logp;
  const double ninf = -HUGE_VAL;
  if (blockIdx.x == 0) {
    double* lf = h.lf;
    for (int s = lane; s < S; s += 64) lf[s] = logp[s] + log(pi[s]);
    for (int t = 1; t <= n; ++t) {
      const double* prev = lf + (int64_t)(t - 1) * S;
      double mx = ninf, sum = 0.0;
      for (int s = lane; s < S; s += 64) mx = fmax(mx, prev[s]);
      mx = chain_max(mx);
      for (int s = lane; s < S; s += 64) sum += exp(prev[s] - mx);
      const double m = mx + log(chain_sum(sum));
      if (lane == 0) h.m[t - 1] = m;
      if (t == n) break;
      for (int s = lane; s < S; s += 64)
        lf[(int64_t)t * S + s] = logp[(int64_t)t * S + s] + logaddexp_d(lnP + prev[s], (ln1mP + log(pi[s])) + m);
    }
  } else {
    double* lb = h.lb;
    for (int s = lane; s < S; s += 64) lb[(int64_t)(n - 1) * S + s] = 0.0;
    for (int t = n - 2; t >= 0; --t) {
      const double* nx = lb + (int64_t)(t + 1) * S;
      const double* lp = logp + (int64_t)(t + 1) * S;
      double mx = ninf, sum = 0.0;
      for (int s = lane; s < S; s += 64) mx = fmax(mx, log(pi[s]) + (lp[s] + nx[s]));
      mx = chain_max(mx);
      for (int s = lane; s < S; s += 64) sum += exp(log(pi[s]) + (lp[s] + nx[s]) - mx);
      const double r = ln1mP + (mx + log(chain_sum(sum)));
      for (int s = lane; s < S; s += 64) lb[(int64_t)t * S + s] = logaddexp_d(lnP + (lp[s] + nx[s]), r);
    }
  }
}

__global__ __launch_bounds__(VB_NT) void vbx_hmm_post_kernel(int n, int S, double* __restrict__ gamma, VbxWs w, VbxHmmWs h) {
  if (*w.done) return;
  const int b = blockIdx.x, t0 = b * VB_ROWS, m = min(VB_ROWS, n - t0);
  const double tll = h.m[n - 1];
  for (int s = threadIdx.x; s < S; s += VB_NT) {
    double acc = 0.0;
    for (int i = 0; i < m; ++i) {
      const int t = t0 + i;
      const int64_t o = (int64_t)t * S + s;
      const double lb = h.lb[o];
      gamma[o] = exp(h.lf[o] + lb - tll);
      if (t > 0) acc += exp(h.m[t - 1] + h.logp[o] + lb - tll);
    }
    h.pipart[(int64_t)b * S + s] = acc;
  }
}

// one block, as vbx_finish_kernel with ii >= 0: ELBO = tll + the M step's sum; pi' = gamma[0] + (1 - P) pi (the partials in block order)
__global__ __launch_bounds__(VB_NT) void vbx_hmm_finish_kernel(int nblk, int n, int S, int ii, double epsilon, double loop_prob,
                                                               const double* __restrict__ gamma, double* __restrict__ pi,
                                                               double* __restrict__ elbo, int32_t* __restrict__ n_iter,
                                                               int32_t* __restrict__ status, VbxWs w, VbxHmmWs h) {
  __shared__ double s_tot;
  if (*w.done) return;
  const int tid = threadIdx.x;
  for (int s = tid; s < S; s += VB_NT) {
    double a = 0.0, p = 0.0;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) a += w.Npart[(int64_t)b * S + s];
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) p += h.pipart[(int64_t)b * S + s];
    w.N[s] = a;
    h.pinew[s] = gamma[s] + ((1.0 - loop_prob) * pi[s]) * p;
  }
  __syncthreads();
  if (tid == 0) {
    double e2 = 0.0, tot = 0.0;
    for (int s = 0; s < S; ++s) e2 += w.es[s];
    for (int s = 0; s < S; ++s) tot += h.pinew[s];
    const double v = h.m[n - 1] + e2;
    elbo[ii] = v;
    *n_iter = ii + 1;
    s_tot = tot;
    const bool fin = isfinite(v);
    if (!fin) atomicOr(status, VB_ST_ELBO);
    if (!fin || (ii > 0 && v - *w.prev < epsilon)) *w.done = 1;
    *w.prev = v;
  }
  __syncthreads();
  for (int s = tid; s < S; s += VB_NT) pi[s] = h.pinew[s] / s_tot;
}

bool vbx_shape_ok(int n, int D, int S) { return n >= 1 && n <= VB_MAX_ROWS && (D == 64 || D == 128) && S >= 1 && S <= VB_MAX_ROWS; }

// carves the workspace (the members of VbxWs in their order); returns its size
size_t vbx_carve(WsCarver c, int n, int D, int S, VbxWs* w) {
  const size_t nblk = (size_t)(n + VB_ROWS - 1) / VB_ROWS, Ss = S, Ds = D;
  *w = VbxWs{c.take<double>(n * Ds),      c.take<double>(n),    c.take<double>(n),       c.take<double>(nblk * Ss), c.take<double>(nblk * Ss * Ds),
             c.take<double>(nblk),        c.take<double>(Ss),   c.take<double>(Ds * Ss), c.take<double>(Ss),        c.take<double>(Ss),
             c.take<double>(1),           c.take<int32_t>(1)};
  return c.bytes();
}

// sdk_vbx_hmm's workspace: sdk_vbx's, then the chain's
size_t vbx_hmm_carve(WsCarver c, int n, int D, int S, VbxWs* w, VbxHmmWs* h) {
  const size_t nblk = (size_t)(n + VB_ROWS - 1) / VB_ROWS, Ss = S;
  c.off = vbx_carve(c, n, D, S, w);
  *h = VbxHmmWs{c.take<double>(n * Ss), c.take<double>(n * Ss), c.take<double>(n * Ss), c.take<double>(n), c.take<double>(nblk * Ss), c.take<double>(Ss)};
  return c.bytes();
}

}  // namespace

extern "C" int sdk_plda_transform(sdk_ctx* ctx, const float* E, int d_in, const int32_t* rows, int n, const double* mean1, const double* lda,
                                  const double* mean2, const double* mu, const double* Tt, int D0, int D, double* X, void* stream) {
  SDK_REQUIRE(ctx, "sdk_plda_transform: null context");
  SDK_REQUIRE(n >= 0 && n <= VB_MAX_ROWS, "sdk_plda_transform: n=%d (0 .. %d)", n, VB_MAX_ROWS);
  SDK_REQUIRE(d_in >= 64 && d_in <= PLDA_MAX_DIM && d_in % 64 == 0, "sdk_plda_transform: d_in=%d not supported (a multiple of 64, at most %d)", d_in,
              PLDA_MAX_DIM);
  SDK_REQUIRE(D0 >= 1 && D0 <= PLDA_MAX_DIM, "sdk_plda_transform: D0=%d (1 .. %d)", D0, PLDA_MAX_DIM);
  SDK_REQUIRE((D == 64 || D == 128) && D <= D0, "sdk_plda_transform: D=%d not supported (64 or 128, at most D0=%d)", D, D0);
  if (n == 0) return 0;
  SDK_REQUIRE(E && rows && mean1 && lda && mean2 && mu && Tt && X, "sdk_plda_transform: null argument (E=%p rows=%p mean1=%p lda=%p mean2=%p mu=%p Tt=%p X=%p)",
              (const void*)E, (const void*)rows, (const void*)mean1, (const void*)lda, (const void*)mean2, (const void*)mu, (const void*)Tt, (void*)X);
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * n * ((double)d_in * D0 + (double)D0 * D), (double)n * (4.0 * d_in + 8.0 * D) + 8.0 * D0 * (d_in + D));
  hipLaunchKernelGGL(plda_transform_kernel, dim3((n + PLDA_RPB - 1) / PLDA_RPB), dim3(PLDA_NT), 0, (hipStream_t)stream, E, d_in, rows, n, mean1, lda, mean2, mu,
                     Tt, D0, D, X);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t sdk_vbx_workspace_bytes(int n, int D, int S) {
  if (!vbx_shape_ok(n, D, S)) {
    sdk_set_error("sdk_vbx_workspace_bytes: n=%d D=%d S=%d (n and S 1 .. %d, D 64 or 128)", n, D, S, VB_MAX_ROWS);
    return 0;
  }
  VbxWs w;
  return vbx_carve({}, n, D, S, &w);
}

extern "C" int sdk_vbx(sdk_ctx* ctx, const double* X, const double* Phi, const int32_t* labels, int n, int D, int S, double Fa, double Fb,
                       int max_iters, double epsilon, double init_smoothing, double* gamma, double* pi, double* elbo, int32_t* n_iter,
                       int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx, "sdk_vbx: null context");
  SDK_REQUIRE(n >= 1 && n <= VB_MAX_ROWS, "sdk_vbx: n=%d (1 .. %d)", n, VB_MAX_ROWS);
  SDK_REQUIRE(D == 64 || D == 128, "sdk_vbx: D=%d not supported (64 or 128)", D);
  SDK_REQUIRE(S >= 1 && S <= VB_MAX_ROWS, "sdk_vbx: S=%d (1 .. %d)", S, VB_MAX_ROWS);
  SDK_REQUIRE(max_iters >= 1 && max_iters <= 1000, "sdk_vbx: max_iters=%d (1 .. 1000)", max_iters);
  SDK_REQUIRE(Fa > 0.0 && Fb > 0.0 && isfinite(Fa) && isfinite(Fb), "sdk_vbx: Fa=%g Fb=%g (positive and finite)", Fa, Fb);
  SDK_REQUIRE(epsilon == epsilon, "sdk_vbx: epsilon is NaN");
  SDK_REQUIRE(init_smoothing >= 0.0 && isfinite(init_smoothing), "sdk_vbx: init_smoothing=%g (finite, at least 0)", init_smoothing);
  SDK_REQUIRE(X && Phi && labels && gamma && pi && elbo && n_iter && status && ws,
              "sdk_vbx: null argument (X=%p Phi=%p labels=%p gamma=%p pi=%p elbo=%p n_iter=%p status=%p ws=%p)", (const void*)X, (const void*)Phi,
              (const void*)labels, (void*)gamma, (void*)pi, (void*)elbo, (void*)n_iter, (void*)status, ws);
  SDK_REQUIRE_WS("sdk_vbx", "sdk_vbx_workspace_bytes", ws, ws_bytes, sdk_vbx_workspace_bytes(n, D, S), 256);
  VbxWs w;
  vbx_carve({static_cast<char*>(ws), 0}, n, D, S, &w);
  const int nblk = (n + VB_ROWS - 1) / VB_ROWS;
  hipStream_t st = (hipStream_t)stream;
  const dim3 gstats(nblk, (S + VB_SC - 1) / VB_SC);
  ProfScope ps(ctx, stream, SDK_K_COPY, 4.0 * max_iters * (double)n * S * D, 16.0 * max_iters * (double)n * (S + D));
  hipLaunchKernelGGL(vbx_reset_kernel, dim3(1), dim3(64), 0, st, S, max_iters, pi, elbo, n_iter, status, w);
  hipLaunchKernelGGL(vbx_init_kernel, dim3((n + 3) / 4), dim3(VB_NT), 0, st, X, Phi, labels, n, D, S, init_smoothing, gamma, status, w);
  hipLaunchKernelGGL(vbx_stats_kernel, gstats, dim3(D), 0, st, gamma, n, D, S, 0, w);
  hipLaunchKernelGGL(vbx_finish_kernel, dim3(1), dim3(VB_NT), 0, st, nblk, S, -1, epsilon, pi, elbo, n_iter, status, w);
  for (int ii = 0; ii < max_iters; ++ii) {
    hipLaunchKernelGGL(vbx_mstep_kernel, dim3(S), dim3(D), 0, st, Phi, nblk, D, S, Fa, Fb, w);
    hipLaunchKernelGGL(vbx_estep_kernel<false>, dim3(nblk), dim3(VB_NT), 0, st, pi, n, D, S, Fa, gamma, w);
    hipLaunchKernelGGL(vbx_stats_kernel, gstats, dim3(D), 0, st, gamma, n, D, S, 1, w);
    hipLaunchKernelGGL(vbx_finish_kernel, dim3(1), dim3(VB_NT), 0, st, nblk, S, ii, epsilon, pi, elbo, n_iter, status, w);
  }
  SDK_LAUNCH_CHECK();
  return 0;
}

// the chain's launch: speakers in registers up to S = 64 VH_MAXK, the memory form above
static void vbx_chain_launch(hipStream_t st, const double* pi, int n, int S, double lnP, double ln1mP, const VbxWs& w, const VbxHmmWs& h) {
  const int K = (S + 63) / 64;
  static_assert(VH_MAXK == 4, "one instantiation per K");
  if (K == 1) hipLaunchKernelGGL(vbx_chain_kernel<1>, dim3(2), dim3(64), 0, st, pi, n, S, lnP, ln1mP, w, h);
  else if (K == 2) hipLaunchKernelGGL(vbx_chain_kernel<2>, dim3(2), dim3(64), 0, st, pi, n, S, lnP, ln1mP, w, h);
  else if (K == 3) hipLaunchKernelGGL(vbx_chain_kernel<3>, dim3(2), dim3(64), 0, st, pi, n, S, lnP, ln1mP, w, h);
  else if (K == 4) hipLaunchKernelGGL(vbx_chain_kernel<4>, dim3(2), dim3(64), 0, st, pi, n, S, lnP, ln1mP, w, h);
  else hipLaunchKernelGGL(vbx_chain_mem_kernel, dim3(2), dim3(64), 0, st, pi, n, S, lnP, ln1mP, w, h);
}

extern "C" size_t sdk_vbx_hmm_workspace_bytes(int n, int D, int S) {
  if (!vbx_shape_ok(n, D, S)) {
    sdk_set_error("sdk_vbx_hmm_workspace_bytes: n=%d D=%d S=%d (n and S 1 .. %d, D 64 or 128)", n, D, S, VB_MAX_ROWS);
    return 0;
  }
  VbxWs w;
  VbxHmmWs h;
  return vbx_hmm_carve({}, n, D, S, &w, &h);
}

extern "C" int sdk_vbx_hmm(sdk_ctx* ctx, const double* X, const double* Phi, const int32_t* labels, int n, int D, int S, double Fa, double Fb,
                           int max_iters, double epsilon, double init_smoothing, double loop_prob, double* gamma, double* pi, double* elbo,
                           int32_t* n_iter, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(loop_prob >= 0.0 && loop_prob < 1.0, "sdk_vbx_hmm: loop_prob=%g (at least 0, below 1)", loop_prob);      // a NaN fails both
  SDK_REQUIRE(ctx, "sdk_vbx_hmm: null context");
  SDK_REQUIRE(n >= 1 && n <= VB_MAX_ROWS, "sdk_vbx_hmm: n=%d (1 .. %d)", n, VB_MAX_ROWS);
  SDK_REQUIRE(D == 64 || D == 128, "sdk_vbx_hmm: D=%d not supported (64 or 128)", D);
  SDK_REQUIRE(S >= 1 && S <= VB_MAX_ROWS, "sdk_vbx_hmm: S=%d (1 .. %d)", S, VB_MAX_ROWS);
  SDK_REQUIRE(max_iters >= 1 && max_iters <= 1000, "sdk_vbx_hmm: max_iters=%d (1 .. 1000)", max_iters);
  SDK_REQUIRE(Fa > 0.0 && Fb > 0.0 && isfinite(Fa) && isfinite(Fb), "sdk_vbx_hmm: Fa=%g Fb=%g (positive and finite)", Fa, Fb);
  SDK_REQUIRE(epsilon == epsilon, "sdk_vbx_hmm: epsilon is NaN");
  SDK_REQUIRE(init_smoothing >= 0.0 && isfinite(init_smoothing), "sdk_vbx_hmm: init_smoothing=%g (finite, at least 0)", init_smoothing);
  SDK_REQUIRE(X && Phi && labels && gamma && pi && elbo && n_iter && status && ws,
              "sdk_vbx_hmm: null argument (X=%p Phi=%p labels=%p gamma=%p pi=%p elbo=%p n_iter=%p status=%p ws=%p)", (const void*)X, (const void*)Phi,
              (const void*)labels, (void*)gamma, (void*)pi, (void*)elbo, (void*)n_iter, (void*)status, ws);
  SDK_REQUIRE_WS("sdk_vbx_hmm", "sdk_vbx_hmm_workspace_bytes", ws, ws_bytes, sdk_vbx_hmm_workspace_bytes(n, D, S), 256);
  VbxWs w;
  VbxHmmWs h;
  vbx_hmm_carve({static_cast<char*>(ws), 0}, n, D, S, &w, &h);
  const int nblk = (n + VB_ROWS - 1) / VB_ROWS;
  const double lnP = log(loop_prob), ln1mP = log1p(-loop_prob);          // loop_prob == 0: -inf and 0
  hipStream_t st = (hipStream_t)stream;
  const dim3 gstats(nblk, (S + VB_SC - 1) / VB_SC);
  ProfScope ps(ctx, stream, SDK_K_COPY, 4.0 * max_iters * (double)n * S * D, 16.0 * max_iters * (double)n * (4.0 * S + D));
  hipLaunchKernelGGL(vbx_reset_kernel, dim3(1), dim3(64), 0, st, S, max_iters, pi, elbo, n_iter, status, w);
  hipLaunchKernelGGL(vbx_init_kernel, dim3((n + 3) / 4), dim3(VB_NT), 0, st, X, Phi, labels, n, D, S, init_smoothing, gamma, status, w);
  hipLaunchKernelGGL(vbx_stats_kernel, gstats, dim3(D), 0, st, gamma, n, D, S, 0, w);
  hipLaunchKernelGGL(vbx_finish_kernel, dim3(1), dim3(VB_NT), 0, st, nblk, S, -1, epsilon, pi, elbo, n_iter, status, w);
  for (int ii = 0; ii < max_iters; ++ii) {
    hipLaunchKernelGGL(vbx_mstep_kernel, dim3(S), dim3(D), 0, st, Phi, nblk, D, S, Fa, Fb, w);
    hipLaunchKernelGGL(vbx_estep_kernel<true>, dim3(nblk), dim3(VB_NT), 0, st, pi, n, D, S, Fa, h.logp, w);
    vbx_chain_launch(st, pi, n, S, lnP, ln1mP, w, h);
    hipLaunchKernelGGL(vbx_hmm_post_kernel, dim3(nblk), dim3(VB_NT), 0, st, n, S, gamma, w, h);
    hipLaunchKernelGGL(vbx_stats_kernel, gstats, dim3(D), 0, st, gamma, n, D, S, 0, w);
    hipLaunchKernelGGL(vbx_hmm_finish_kernel, dim3(1), dim3(VB_NT), 0, st, nblk, n, S, ii, epsilon, loop_prob, gamma, pi, elbo, n_iter, status, w, h);
  }
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_vbx_centroids(sdk_ctx* ctx, const double* gamma, const double* pi, const float* E, const int32_t* rows, int n, int S, int d,
                                 int32_t* K, int32_t* keep, int32_t* labels, float* cent, double* cent64, void* stream) {
  SDK_REQUIRE(ctx, "sdk_vbx_centroids: null context");
  SDK_REQUIRE(n >= 1 && n <= VB_MAX_ROWS && S >= 1 && S <= VB_MAX_ROWS, "sdk_vbx_centroids: n=%d S=%d (each 1 .. %d)", n, S, VB_MAX_ROWS);
  SDK_REQUIRE(d >= 64 && d <= PLDA_MAX_DIM && d % 64 == 0, "sdk_vbx_centroids: d=%d not supported (a multiple of 64, at most %d)", d, PLDA_MAX_DIM);
  SDK_REQUIRE(gamma && pi && E && rows && K && keep && cent && cent64,
              "sdk_vbx_centroids: null argument (gamma=%p pi=%p E=%p rows=%p K=%p keep=%p cent=%p cent64=%p)", (const void*)gamma, (const void*)pi,
              (const void*)E, (const void*)rows, (void*)K, (void*)keep, (void*)cent, (void*)cent64);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * n * (double)d * S, (double)S * n * (4.0 * d + 12.0) + 12.0 * S * d);
  hipLaunchKernelGGL(vbx_keep_kernel, dim3(1), dim3(64), 0, st, pi, S, K, keep);
  if (labels) hipLaunchKernelGGL(vbx_labels_kernel, dim3((n + VB_NT - 1) / VB_NT), dim3(VB_NT), 0, st, gamma, n, S, K, keep, labels);
  hipLaunchKernelGGL(vbx_centroids_kernel, dim3(S), dim3(VB_NT), 0, st, gamma, E, rows, n, S, d, K, keep, cent, cent64);
  SDK_LAUNCH_CHECK();
  return 0;
}
