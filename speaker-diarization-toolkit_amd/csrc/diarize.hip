// Speaker diarization (diarize.py): the stages that join the segmentation model, the ResNet34 embedding and the clustering.
//
//   powerset_decode_kernel     logp [C][F][7] -> cls [C][F]: the argmax class, ties to the lower class.  Everything later reads cls.
//   diarize_masks_kernel       cls [B][F] -> the pooling weights of sdk_resnet_forward_masked, w [B][3][T4], and info [B][3][4] per
//                              (chunk, local speaker): (active frames, clean frames, used_clean, valid).
//   diarize_reconstruct_kernel cls, chunk starts, labels [C][3] -> count [G], speakers [G][2] (and act [G][K]) on the global frame grid of
//                              segmentation.aggregate_counts.
//   diarize_centroids_kernel   unit rows E, training rows and their cluster labels -> the clusters' unit centroids (float64 sums in row order).
//   diarize_assign_kernel      E, info, centroids -> labels [C][3] and score [C][3]: every candidate row to the centroid of largest cosine, or
//                              (constrained) the one-to-one matching of a chunk's candidates to clusters with the largest total cosine.
//
// Every kernel is a gather: one owner per output element, no atomics, every sum in a fixed order (the first three kernels are integer
// arithmetic: the weights are 0 / 1), so the results are bit-identical run to run.
#include "common.hpp"
#include "diarize_assign.hpp"

namespace {

constexpr int DZ_NT = 256;
constexpr int DZ_MIN_CLEAN = 4;      // columns of the last map a speaker needs alone before the overlapped ones are dropped (diarize.MIN_CLEAN_COLUMNS)

__global__ __launch_bounds__(DZ_NT) void powerset_decode_kernel(const float* __restrict__ logp, int64_t n, uint8_t* __restrict__ cls) {
  const int64_t i = (int64_t)blockIdx.x * DZ_NT + threadIdx.x;
  if (i >= n) return;
  const float* p = logp + i * 7;
  int best = 0;
  float bv = p[0];
#pragma unroll
  for (int c = 1; c < 7; ++c) {
    const float v = p[c];
    if (v > bv) { bv = v; best = c; }
  }
  cls[i] = (uint8_t)best;
}

// one wave per chunk: frame totals and column totals as integer wave sums, then the weights
__global__ __launch_bounds__(64) void diarize_masks_kernel(const uint8_t* __restrict__ cls, int F, int T4, float* __restrict__ w, int32_t* __restrict__ info) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const uint8_t* c = cls + (int64_t)b * F;
  int act[3] = {0, 0, 0}, cln[3] = {0, 0, 0}, colf[3] = {0, 0, 0}, colc[3] = {0, 0, 0};
  for (int i = lane; i < F; i += 64) {
    const int m = cls_mask(c[i]);
    const bool alone = __popc(m) < 2;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int a = (m >> s) & 1;
      act[s] += a;
      cln[s] += a & (int)alone;
    }
  }
  for (int j = lane; j < T4; j += 64) {
    const int i = min(F - 1, (int)(((int64_t)j * F) / T4));
    const int m = cls_mask(c[i]);
    const bool alone = __popc(m) < 2;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int a = (m >> s) & 1;
      colf[s] += a;
      colc[s] += a & (int)alone;
    }
  }
  bool use_clean[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    act[s] = wave_sum(act[s]);
    cln[s] = wave_sum(cln[s]);
    colf[s] = wave_sum(colf[s]);
    colc[s] = wave_sum(colc[s]);
    use_clean[s] = colc[s] >= DZ_MIN_CLEAN;
    if (lane == 0) {
      int32_t* o = info + ((int64_t)b * 3 + s) * 4;
      o[0] = act[s];
      o[1] = cln[s];
      o[2] = use_clean[s];
      o[3] = (use_clean[s] ? colc[s] : colf[s]) >= 2;
    }
  }
  for (int j = lane; j < T4; j += 64) {
    const int i = min(F - 1, (int)(((int64_t)j * F) / T4));
    const int m = cls_mask(c[i]);
    const bool alone = __popc(m) < 2;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const bool a = (m >> s) & 1;
      w[((int64_t)b * 3 + s) * T4 + j] = (a && (alone || !use_clean[s])) ? 1.f : 0.f;
    }
  }
}

// thread = one global frame.  The starts ascend, so q_c never grows with c: the chunks with g + q_c >= 0 are a prefix, those with
// g + q_c < F a suffix, and the chunks that see the frame are the range between two binary searches.
// Frame g of a recording whose chunks are cb .. ce - 1 of cls / starts / labels; count, speakers and act point at the frame's own elements.
__device__ __forceinline__ void reconstruct_frame(const uint8_t* __restrict__ cls, const int32_t* __restrict__ starts,
                                                  const int32_t* __restrict__ labels, int cb, int ce, int F, int K, int g, int max_speakers,
                                                  uint8_t* __restrict__ count, int32_t* __restrict__ speakers, int32_t* __restrict__ act) {
  int lo = cb, hi = ce;                                // first chunk with g + q_c < F
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g + chunk_q(starts[mid]) < F) hi = mid; else lo = mid + 1;
  }
  const int c0 = lo;
  lo = cb; hi = ce;                                    // first chunk with g + q_c < 0
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g + chunk_q(starts[mid]) < 0) hi = mid; else lo = mid + 1;
  }
  const int c1 = lo;                                   // chunks c0 .. c1 - 1 see the frame
  int nc = 0, cnt = 0;
  for (int c = c0; c < c1; ++c) {
    const int i = g + (int)chunk_q(starts[c]);
    if ((unsigned)i >= (unsigned)F) continue;           // starts that do not ascend: never read outside the chunk
    cnt += __popc(cls_mask(cls[(int64_t)c * F + i]));
    ++nc;
  }
  int a1 = 0, k1 = -1, a2 = 0, k2 = -1;                // the two largest act > 0, ties to the lower cluster
  for (int k = 0; k < K; ++k) {
    int a = 0;
    for (int c = c0; c < c1; ++c) {
      const int i = g + (int)chunk_q(starts[c]);
      if ((unsigned)i >= (unsigned)F) continue;
      const int m = cls_mask(cls[(int64_t)c * F + i]);
      const int32_t* lb = labels + (int64_t)c * 3;
      a += (int)(((m & 1) && lb[0] == k) || ((m & 2) && lb[1] == k) || ((m & 4) && lb[2] == k));
    }
    if (act) act[k] = a;
    if (a > a1) { a2 = a1; k2 = k1; a1 = a; k1 = k; }
    else if (a > a2) { a2 = a; k2 = k; }
  }
  int n = nc ? (2 * cnt + nc) / (2 * nc) : 0;           // the mean count, rounded half up
  n = min(n, min(2, max_speakers));
  *count = (uint8_t)n;
  speakers[0] = n >= 1 ? k1 : -1;
  speakers[1] = n >= 2 ? k2 : -1;
}

__global__ __launch_bounds__(DZ_NT) void diarize_reconstruct_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ starts,
                                                                    const int32_t* __restrict__ labels, int C, int F, int K, int G, int max_speakers,
                                                                    uint8_t* __restrict__ count, int32_t* __restrict__ speakers,
                                                                    int32_t* __restrict__ act) {
  const int g = blockIdx.x * DZ_NT + threadIdx.x;
  if (g >= G) return;
  reconstruct_frame(cls, starts, labels, 0, C, F, K, g, max_speakers, count + g, speakers + 2 * (int64_t)g, act ? act + (int64_t)g * K : nullptr);
}

// ---- assignment (diarize.py "assignment"): centroids of the training rows, then every candidate row to a centroid ------------------------
constexpr int DZ_TILE = 256;         // (row, label) pairs staged in LDS per step of the centroid sum

// block = one cluster k, thread = the columns tid, tid + 256.  The n (row, label) pairs pass through LDS in tiles; every thread walks them in
// ascending order and adds the rows labelled k in float64, so a column's sum has one owner and one order.  Then mean, norm (block_sum of
// the squares, reduce.hpp), unit row.  A cluster without rows gives a zero row.
__global__ __launch_bounds__(DZ_NT) void diarize_centroids_kernel(const float* __restrict__ E, const int32_t* __restrict__ rows,
                                                                  const int32_t* __restrict__ labels, int n, int d, float* __restrict__ cent,
                                                                  double* __restrict__ cent64) {
  __shared__ int32_t s_row[DZ_TILE];
  __shared__ int32_t s_lab[DZ_TILE];
  __shared__ double s_red[DZ_NT / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int j0 = tid, j1 = tid + DZ_NT;
  double a0 = 0.0, a1 = 0.0;
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += DZ_TILE) {
    const int m = min(DZ_TILE, n - i0);
    __syncthreads();
    if (tid < m) {
      s_row[tid] = rows[i0 + tid];
      s_lab[tid] = labels[i0 + tid];
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {
      if (s_lab[i] != k) continue;                     // uniform over the block
      const float* e = E + (int64_t)s_row[i] * d;
      ++cnt;
      if (j0 < d) a0 += (double)e[j0];
      if (j1 < d) a1 += (double)e[j1];
    }
  }
  if (cnt) { a0 /= (double)cnt; a1 /= (double)cnt; }
  const double nrm = fmax(sqrt(block_sum((j0 < d ? a0 * a0 : 0.0) + (j1 < d ? a1 * a1 : 0.0), s_red)), 1e-300);
  a0 /= nrm;
  a1 /= nrm;
  if (j0 < d) {
    cent[(int64_t)k * d + j0] = (float)a0;
    if (cent64) cent64[(int64_t)k * d + j0] = a0;
  }
  if (j1 < d) {
    cent[(int64_t)k * d + j1] = (float)a1;
    if (cent64) cent64[(int64_t)k * d + j1] = a1;
  }
}

// one wave per chunk: the chunk's candidate rows go to LDS, the wave solves the assignment (diarize_assign.hpp), lane 0 writes the chunk's
// three labels and scores
__device__ __forceinline__ void assign_chunk(const float* __restrict__ E, const int32_t* __restrict__ info, const double* __restrict__ cent, int K,
                                             int d, int constrained, int32_t* __restrict__ labels, float* __restrict__ score, int c) {
  __shared__ AssignLds L;
  const int lane = threadIdx.x;
  bool cand[3];
  assign_candidates(info + (int64_t)c * 12, cand);
  assign_stage(L, E + (int64_t)c * 3 * d, cand, d, lane, 64);
  __syncthreads();
  int32_t lab[3];
  double cosv[3];
  assign_solve(L, cand, cent, K, d, constrained, lane, lab, cosv);
  if (lane != 0) return;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    labels[(int64_t)c * 3 + s] = lab[s];
    score[(int64_t)c * 3 + s] = (float)cosv[s];
  }
}

__global__ __launch_bounds__(64) void diarize_assign_kernel(const float* __restrict__ E, const int32_t* __restrict__ info,
                                                            const double* __restrict__ cent, int K, int d, int constrained,
                                                            int32_t* __restrict__ labels, float* __restrict__ score) {
  assign_chunk(E, info, cent, K, d, constrained, labels, score, blockIdx.x);
}

// ---- many recordings in one pass (diarize.Diarizer.run_many): R recordings laid end to end.  chunk_off, frame_off and cent_off [R + 1] are
// the prefix sums of their chunks, global frames and clusters; a kernel finds the recording of its element by a binary search on the table
// that counts such elements (packed_grid.hpp's pg_find_group; no per-element table is built).  Every output element has one owner and every
// sum a fixed order, as above.

// one wave per chunk, the rule of diarize_assign_kernel on the centroids of the chunk's own recording; labels are local to the recording
__global__ __launch_bounds__(64) void diarize_assign_grouped_kernel(const float* __restrict__ E, const int32_t* __restrict__ info,
                                                                    const double* __restrict__ cent, const int32_t* __restrict__ chunk_off,
                                                                    const int32_t* __restrict__ cent_off, int R, int d, int constrained,
                                                                    int32_t* __restrict__ labels, float* __restrict__ score) {
  const int c = blockIdx.x;
  const int r = pg_find_group(chunk_off, R, c);
  const int k0 = cent_off[r], K = cent_off[r + 1] - k0;
  if (K <= 0) {                                        // uniform over the wave: a recording without clusters
    if (threadIdx.x < 3) {
      labels[(int64_t)c * 3 + threadIdx.x] = -1;
      score[(int64_t)c * 3 + threadIdx.x] = 0.f;
    }
    return;
  }
  assign_chunk(E, info, cent + (int64_t)k0 * d, K, d, constrained, labels, score, c);
}

// one wave per cluster k of the cut (cluster.fold_small_clusters, steps 2 - 4).  A large cluster (sizes >= eff of its recording) stays; a small
// one goes to the large cluster of its recording with the largest cosine - unit float64 centroids, one fma chain per pair in column order,
// lane l takes the clusters l, l + 64, .. - ties to the lower cluster; a recording without a large cluster sends everything to its first.
__global__ __launch_bounds__(64) void diarize_fold_target_kernel(const double* __restrict__ cent, const int32_t* __restrict__ sizes,
                                                                 const int32_t* __restrict__ cl_off, const int32_t* __restrict__ eff, int R, int d,
                                                                 int32_t* __restrict__ target) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int r = pg_find_group(cl_off, R, k);
  const int b = cl_off[r], e = cl_off[r + 1], m = eff[r];
  if (sizes[k] >= m) {
    if (lane == 0) target[k] = k;
    return;
  }
  const double* ck = cent + (int64_t)k * d;
  double bv = 0.0;
  int bk = -1, fl = INT32_MAX;                         // fl: the first large cluster (taken when every cosine is a NaN)
  for (int j = b + lane; j < e; j += 64) {
    if (sizes[j] < m) continue;
    fl = min(fl, j);
    const double* cj = cent + (int64_t)j * d;
    double a = 0.0;
    for (int i = 0; i < d; ++i) a = fma(ck[i], cj[i], a);
    if (a == a && better(a, j, bv, bk)) { bv = a; bk = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int ok = __shfl_xor(bk, o, 64);
    fl = min(fl, __shfl_xor(fl, o, 64));
    if (ok >= 0 && better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
  }
  if (lane == 0) target[k] = bk >= 0 ? bk : (fl != INT32_MAX ? fl : b);
}

// thread = recording: the kept clusters numbered by first appearance.  The cut's labels are canonical, so cluster j first appears before
// cluster j + 1 and a kept cluster's first appearance is the lowest j sent to it: one ascending walk.  remap[j] = cent_off[r] + new number.
__global__ __launch_bounds__(DZ_NT) void diarize_fold_number_kernel(const int32_t* __restrict__ target, const int32_t* __restrict__ cl_off,
                                                                    const int32_t* __restrict__ cent_off, int R, int32_t* __restrict__ remap) {
  const int r = blockIdx.x * DZ_NT + threadIdx.x;
  if (r >= R) return;
  const int b = cl_off[r], e = cl_off[r + 1];
  const int last = cent_off[r + 1] - 1;
  int next = cent_off[r];
  for (int j = b; j < e; ++j) remap[j] = -1;
  for (int j = b; j < e; ++j) {
    const int t = target[j];                           // a kept cluster of this recording (its own target)
    if (remap[t] < 0) { remap[t] = min(next, last); ++next; }
  }
  for (int j = b; j < e; ++j) {
    const int t = target[j];
    if (t != j) remap[j] = remap[t];
  }
}

__global__ __launch_bounds__(DZ_NT) void diarize_fold_apply_kernel(const int32_t* __restrict__ remap, const int32_t* __restrict__ cut, int n,
                                                                   int Kc, int32_t* __restrict__ out) {
  const int i = blockIdx.x * DZ_NT + threadIdx.x;
  if (i >= n) return;
  const int c = cut[i];
  out[i] = (unsigned)c < (unsigned)Kc ? remap[c] : -1;
}

// thread = packed frame
__global__ __launch_bounds__(DZ_NT) void diarize_reconstruct_grouped_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ starts,
                                                                            const int32_t* __restrict__ labels, const int32_t* __restrict__ chunk_off,
                                                                            const int32_t* __restrict__ frame_off, const int64_t* __restrict__ n_samples,
                                                                            const int32_t* __restrict__ cent_off, int R, int F, int G, int max_speakers,
                                                                            uint8_t* __restrict__ count, int32_t* __restrict__ speakers,
                                                                            int32_t* __restrict__ act, const int64_t* __restrict__ act_off) {
  const int gp = blockIdx.x * DZ_NT + threadIdx.x;
  if (gp >= G) return;
  const int r = pg_find_group(frame_off, R, gp);
  const int g = gp - frame_off[r];
  const int K = max(cent_off[r + 1] - cent_off[r], 1);  // no cluster: one cluster that no label names
  if (g >= dz_frames(n_samples[r])) {                   // a frame table longer than the recording: no chunk sees the frame
    count[gp] = 0;
    speakers[2 * (int64_t)gp] = speakers[2 * (int64_t)gp + 1] = -1;
    return;
  }
  reconstruct_frame(cls, starts, labels, chunk_off[r], chunk_off[r + 1], F, K, g, max_speakers, count + gp, speakers + 2 * (int64_t)gp,
                    act ? act + act_off[r] + (int64_t)g * K : nullptr);
}

__global__ __launch_bounds__(DZ_NT) void fill_i32_kernel(int32_t* __restrict__ p, int n, int32_t v) {
  const int i = blockIdx.x * DZ_NT + threadIdx.x;
  if (i < n) p[i] = v;
}

// thread = (packed frame, slot): an integer atomicMin of 2 g + slot on the cluster named there; the minimum does not depend on the order
__global__ __launch_bounds__(DZ_NT) void diarize_first_seen_kernel(const int32_t* __restrict__ speakers, const int32_t* __restrict__ frame_off,
                                                                   const int32_t* __restrict__ cent_off, int R, int G, int32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * DZ_NT + threadIdx.x;
  if (i >= 2 * (int64_t)G) return;
  const int k = speakers[i];
  if (k < 0) return;
  const int gp = (int)(i >> 1);
  const int r = pg_find_group(frame_off, R, gp);
  if (k >= cent_off[r + 1] - cent_off[r]) return;
  atomicMin(first + cent_off[r] + k, 2 * (gp - frame_off[r]) + (int)(i & 1));
}

// thread = cluster: its rank among (first, k) of its recording
__global__ __launch_bounds__(DZ_NT) void diarize_rank_kernel(const int32_t* __restrict__ first, const int32_t* __restrict__ cent_off, int R, int K,
                                                             int32_t* __restrict__ renum) {
  const int k = blockIdx.x * DZ_NT + threadIdx.x;
  if (k >= K) return;
  const int r = pg_find_group(cent_off, R, k);
  const int f = first[k];
  int n = 0;
  for (int j = cent_off[r]; j < cent_off[r + 1]; ++j) {
    const int fj = first[j];
    n += (int)(fj < f || (fj == f && j < k));
  }
  renum[k] = n;
}

__global__ __launch_bounds__(DZ_NT) void diarize_relabel_kernel(const int32_t* __restrict__ renum, const int32_t* __restrict__ chunk_off,
                                                                const int32_t* __restrict__ cent_off, int R, int C, int32_t* __restrict__ labels) {
  const int i = blockIdx.x * DZ_NT + threadIdx.x;
  if (i >= 3 * C) return;
  const int l = labels[i];
  if (l < 0) return;
  const int r = pg_find_group(chunk_off, R, i / 3);
  if (l < cent_off[r + 1] - cent_off[r]) labels[i] = renum[cent_off[r] + l];
}

// block = cluster: its fp32 and float64 centroid rows go to their new place (out of place)
__global__ __launch_bounds__(DZ_NT) void diarize_permute_kernel(const int32_t* __restrict__ renum, const int32_t* __restrict__ cent_off, int R, int d,
                                                                const float* __restrict__ c32, const double* __restrict__ c64,
                                                                float* __restrict__ o32, double* __restrict__ o64) {
  const int k = blockIdx.x;
  const int r = pg_find_group(cent_off, R, k);
  const int64_t dst = (int64_t)(cent_off[r] + renum[k]) * d, src = (int64_t)k * d;
  for (int j = threadIdx.x; j < d; j += DZ_NT) {
    o32[dst + j] = c32[src + j];
    o64[dst + j] = c64[src + j];
  }
}

}  // namespace

extern "C" int sdk_powerset_decode(sdk_ctx* ctx, const float* logp, int C, int F, uint8_t* cls, void* stream) {
  SDK_REQUIRE(ctx, "sdk_powerset_decode: null context");
  SDK_REQUIRE(C >= 0 && F >= 0, "sdk_powerset_decode: C=%d F=%d", C, F);
  const int64_t n = (int64_t)C * F;
  if (n == 0) return 0;
  SDK_REQUIRE(logp && cls, "sdk_powerset_decode: null argument (logp=%p cls=%p)", (const void*)logp, (void*)cls);
  SDK_REQUIRE(n < (1ll << 31) - DZ_NT, "sdk_powerset_decode: C*F=%lld frames (at most 2^31 - %d per call)", (long long)n, DZ_NT + 1);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 29.0 * n);
  hipLaunchKernelGGL(powerset_decode_kernel, dim3((unsigned)((n + DZ_NT - 1) / DZ_NT)), dim3(DZ_NT), 0, (hipStream_t)stream, logp, n, cls);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_diarize_masks(sdk_ctx* ctx, const uint8_t* cls, int B, int F, int T4, float* w, int32_t* info, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_masks: null context");
  SDK_REQUIRE(B >= 0 && F >= 1 && T4 >= 1, "sdk_diarize_masks: B=%d F=%d T4=%d (F and T4 at least 1)", B, F, T4);
  if (B == 0) return 0;
  SDK_REQUIRE(cls && w && info, "sdk_diarize_masks: null argument (cls=%p w=%p info=%p)", (const void*)cls, (void*)w, (void*)info);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)B * (F + 12.0 * T4 + 48.0));
  hipLaunchKernelGGL(diarize_masks_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, cls, F, T4, w, info);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t sdk_diarize_frames(int64_t n_samples) { return dz_frames(n_samples); }

extern "C" int sdk_diarize_reconstruct(sdk_ctx* ctx, const uint8_t* cls, const int32_t* starts, const int32_t* labels, int C, int F, int K,
                                       int64_t n_samples, int max_speakers, uint8_t* count, int32_t* speakers, int32_t* act, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_reconstruct: null context");
  SDK_REQUIRE(C >= 1 && F >= 1 && K >= 1, "sdk_diarize_reconstruct: C=%d F=%d K=%d (each at least 1)", C, F, K);
  SDK_REQUIRE(max_speakers >= 0, "sdk_diarize_reconstruct: max_speakers=%d (0, 1 or 2; larger values do not bind: the powerset bounds the count by 2)", max_speakers);
  const int64_t G = sdk_diarize_frames(n_samples);
  if (G == 0) return 0;
  SDK_REQUIRE(cls && starts && labels && count && speakers, "sdk_diarize_reconstruct: null argument");
  SDK_REQUIRE(G < (1ll << 31) - DZ_NT && (!act || G * K < (1ll << 40)), "sdk_diarize_reconstruct: n_samples=%lld gives %lld frames (at most 2^31 - %d)",
              (long long)n_samples, (long long)G, DZ_NT + 1);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)G * (9.0 + (act ? 4.0 * K : 0.0)) + (double)C * (F + 20.0));
  hipLaunchKernelGGL(diarize_reconstruct_kernel, dim3((unsigned)((G + DZ_NT - 1) / DZ_NT)), dim3(DZ_NT), 0, (hipStream_t)stream, cls, starts, labels, C, F, K,
                     (int)G, max_speakers, count, speakers, act);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_diarize_centroids(sdk_ctx* ctx, const float* E, const int32_t* rows, const int32_t* labels, int n, int K, int d, float* cent,
                                     double* cent64, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_centroids: null context");
  SDK_REQUIRE(n >= 0 && K >= 1, "sdk_diarize_centroids: n=%d K=%d (n at least 0, K at least 1)", n, K);
  SDK_REQUIRE(d >= 64 && d <= DZ_MAX_D && d % 64 == 0, "sdk_diarize_centroids: d=%d not supported (a multiple of 64, at most %d)", d, DZ_MAX_D);
  SDK_REQUIRE(cent && (n == 0 || (E && rows && labels)), "sdk_diarize_centroids: null argument (E=%p rows=%p labels=%p cent=%p)", (const void*)E,
              (const void*)rows, (const void*)labels, (void*)cent);
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * n * d, (double)n * (4.0 * d + 8.0 * K) + 12.0 * K * d);
  hipLaunchKernelGGL(diarize_centroids_kernel, dim3(K), dim3(DZ_NT), 0, (hipStream_t)stream, E, rows, labels, n, d, cent, cent64);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_diarize_assign(sdk_ctx* ctx, const float* E, const int32_t* info, const double* cent64, int C, int K, int d, int constrained,
                                  int32_t* labels, float* score, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_assign: null context");
  SDK_REQUIRE(C >= 0 && K >= 1, "sdk_diarize_assign: C=%d K=%d (C at least 0, K at least 1)", C, K);
  SDK_REQUIRE(d >= 64 && d <= DZ_MAX_D && d % 64 == 0, "sdk_diarize_assign: d=%d not supported (a multiple of 64, at most %d)", d, DZ_MAX_D);
  SDK_REQUIRE(constrained == 0 || constrained == 1, "sdk_diarize_assign: constrained=%d (0 or 1)", constrained);
  if (C == 0) return 0;
  SDK_REQUIRE(E && info && cent64 && labels && score, "sdk_diarize_assign: null argument (E=%p info=%p cent64=%p labels=%p score=%p)", (const void*)E,
              (const void*)info, (const void*)cent64, (void*)labels, (void*)score);
  SDK_REQUIRE(((uintptr_t)cent64 & 15) == 0, "sdk_diarize_assign: cent64=%p must be 16-byte aligned", (const void*)cent64);
  ProfScope ps(ctx, stream, SDK_K_COPY, 6.0 * C * K * d, (double)C * (12.0 * d + 72.0) + 8.0 * K * d);
  hipLaunchKernelGGL(diarize_assign_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, E, info, cent64, K, d, constrained, labels, score);
  SDK_LAUNCH_CHECK();
  return 0;
}

// ---- many recordings in one pass: the offset tables are DEVICE arrays (the kernels search them); the totals come as arguments
#define DZ_GRID(n) pg_grid(n, DZ_NT)

extern "C" int sdk_diarize_assign_grouped(sdk_ctx* ctx, const float* E, const int32_t* info, const double* cent64, const int32_t* chunk_off,
                                          const int32_t* cent_off, int R, int C, int d, int constrained, int32_t* labels, float* score, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_assign_grouped: null context");
  SDK_REQUIRE(R >= 1 && C >= 0, "sdk_diarize_assign_grouped: R=%d C=%d (R at least 1, C at least 0)", R, C);
  SDK_REQUIRE(d >= 64 && d <= DZ_MAX_D && d % 64 == 0, "sdk_diarize_assign_grouped: d=%d not supported (a multiple of 64, at most %d)", d, DZ_MAX_D);
  SDK_REQUIRE(constrained == 0 || constrained == 1, "sdk_diarize_assign_grouped: constrained=%d (0 or 1)", constrained);
  if (C == 0) return 0;
  SDK_REQUIRE(E && info && cent64 && chunk_off && cent_off && labels && score,
              "sdk_diarize_assign_grouped: null argument (E=%p info=%p cent64=%p chunk_off=%p cent_off=%p labels=%p score=%p)", (const void*)E,
              (const void*)info, (const void*)cent64, (const void*)chunk_off, (const void*)cent_off, (void*)labels, (void*)score);
  SDK_REQUIRE(((uintptr_t)cent64 & 15) == 0, "sdk_diarize_assign_grouped: cent64=%p must be 16-byte aligned", (const void*)cent64);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)C * (12.0 * d + 72.0));
  hipLaunchKernelGGL(diarize_assign_grouped_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, E, info, cent64, chunk_off, cent_off, R, d, constrained,
                     labels, score);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_diarize_fold_grouped(sdk_ctx* ctx, const double* cent64, const int32_t* sizes, const int32_t* cl_off, const int32_t* eff,
                                        const int32_t* cent_off, int R, int Kc, int d, int32_t* target, int32_t* remap, const int32_t* cut, int n,
                                        int32_t* out, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_fold_grouped: null context");
  SDK_REQUIRE(R >= 1 && Kc >= 0 && n >= 0, "sdk_diarize_fold_grouped: R=%d Kc=%d n=%d (R at least 1, Kc and n at least 0)", R, Kc, n);
  SDK_REQUIRE(d >= 64 && d <= DZ_MAX_D && d % 64 == 0, "sdk_diarize_fold_grouped: d=%d not supported (a multiple of 64, at most %d)", d, DZ_MAX_D);
  if (Kc == 0) return 0;
  SDK_REQUIRE(cent64 && sizes && cl_off && eff && cent_off && target && remap && (n == 0 || (cut && out)),
              "sdk_diarize_fold_grouped: null argument (cent64=%p sizes=%p cl_off=%p eff=%p cent_off=%p target=%p remap=%p cut=%p out=%p)",
              (const void*)cent64, (const void*)sizes, (const void*)cl_off, (const void*)eff, (const void*)cent_off, (void*)target, (void*)remap,
              (const void*)cut, (void*)out);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)Kc * (8.0 * d + 16.0) + 8.0 * n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(diarize_fold_target_kernel, dim3(Kc), dim3(64), 0, s, cent64, sizes, cl_off, eff, R, d, target);
  SDK_LAUNCH_CHECK();
  hipLaunchKernelGGL(diarize_fold_number_kernel, DZ_GRID(R), dim3(DZ_NT), 0, s, (const int32_t*)target, cl_off, cent_off, R, remap);
  SDK_LAUNCH_CHECK();
  if (n) {
    hipLaunchKernelGGL(diarize_fold_apply_kernel, DZ_GRID(n), dim3(DZ_NT), 0, s, (const int32_t*)remap, cut, n, Kc, out);
    SDK_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int sdk_diarize_reconstruct_grouped(sdk_ctx* ctx, const uint8_t* cls, const int32_t* starts_local, const int32_t* labels,
                                               const int32_t* chunk_off, const int32_t* frame_off, const int64_t* n_samples, const int32_t* cent_off,
                                               int R, int C, int F, int64_t G, int max_speakers, uint8_t* count, int32_t* speakers, int32_t* act,
                                               const int64_t* act_off, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_reconstruct_grouped: null context");
  SDK_REQUIRE(R >= 1 && C >= 0 && F >= 1 && G >= 0, "sdk_diarize_reconstruct_grouped: R=%d C=%d F=%d G=%lld (R and F at least 1)", R, C, F, (long long)G);
  SDK_REQUIRE(max_speakers >= 0, "sdk_diarize_reconstruct_grouped: max_speakers=%d (0, 1 or 2; larger values do not bind)", max_speakers);
  if (G == 0) return 0;
  SDK_REQUIRE(cls && starts_local && labels && chunk_off && frame_off && n_samples && cent_off && count && speakers && (!act || act_off),
              "sdk_diarize_reconstruct_grouped: null argument");
  SDK_REQUIRE(G < (1ll << 30), "sdk_diarize_reconstruct_grouped: %lld packed frames (fewer than 2^30)", (long long)G);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)G * 9.0 + (double)C * (F + 20.0));
  hipLaunchKernelGGL(diarize_reconstruct_grouped_kernel, DZ_GRID(G), dim3(DZ_NT), 0, (hipStream_t)stream, cls, starts_local, labels, chunk_off, frame_off,
                     n_samples, cent_off, R, F, (int)G, max_speakers, count, speakers, act, act_off);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_diarize_first_seen(sdk_ctx* ctx, const int32_t* speakers, const int32_t* frame_off, const int32_t* cent_off, int R, int64_t G,
                                      int K, int32_t* first, void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_first_seen: null context");
  SDK_REQUIRE(R >= 1 && G >= 0 && K >= 0 && G < (1ll << 30), "sdk_diarize_first_seen: R=%d G=%lld K=%d (R at least 1, fewer than 2^30 frames)", R,
              (long long)G, K);
  if (K == 0) return 0;
  SDK_REQUIRE(first && cent_off && (G == 0 || (speakers && frame_off)), "sdk_diarize_first_seen: null argument");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 8.0 * G + 4.0 * K);
  hipLaunchKernelGGL(fill_i32_kernel, DZ_GRID(K), dim3(DZ_NT), 0, (hipStream_t)stream, first, K, INT32_MAX);
  SDK_LAUNCH_CHECK();
  if (G) {
    hipLaunchKernelGGL(diarize_first_seen_kernel, DZ_GRID(2 * G), dim3(DZ_NT), 0, (hipStream_t)stream, speakers, frame_off, cent_off, R, (int)G, first);
    SDK_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int sdk_diarize_renumber(sdk_ctx* ctx, const int32_t* first, const int32_t* cent_off, const int32_t* chunk_off, int R, int K, int C, int d,
                                    int32_t* renum, int32_t* labels, const float* cent, const double* cent64, float* cent_out, double* cent64_out,
                                    void* stream) {
  SDK_REQUIRE(ctx, "sdk_diarize_renumber: null context");
  SDK_REQUIRE(R >= 1 && K >= 0 && C >= 0 && d >= 1, "sdk_diarize_renumber: R=%d K=%d C=%d d=%d", R, K, C, d);
  if (K == 0) return 0;
  SDK_REQUIRE(first && cent_off && renum && (C == 0 || (chunk_off && labels)) && cent && cent64 && cent_out && cent64_out && cent != cent_out &&
              cent64 != cent64_out, "sdk_diarize_renumber: null argument, or centroids permuted in place");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 24.0 * K * d + 24.0 * C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(diarize_rank_kernel, DZ_GRID(K), dim3(DZ_NT), 0, s, first, cent_off, R, K, renum);
  SDK_LAUNCH_CHECK();
  if (C) {
    hipLaunchKernelGGL(diarize_relabel_kernel, DZ_GRID(3 * (int64_t)C), dim3(DZ_NT), 0, s, (const int32_t*)renum, chunk_off, cent_off, R, C, labels);
    SDK_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(diarize_permute_kernel, dim3(K), dim3(DZ_NT), 0, s, (const int32_t*)renum, cent_off, R, d, cent, cent64, cent_out, cent64_out);
  SDK_LAUNCH_CHECK();
  return 0;
}
