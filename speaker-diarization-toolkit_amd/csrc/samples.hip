// Speaker samples (samples.py): each diarized speaker's clean stretches of audio, on the packed frame grid (packed_grid.hpp),
// and the scores of the clips cut from them.
//
//   sdk_samples_runs    speakers [G][2] -> run_off [R + 1], rows [N][4] int32 = (speaker, g0, g1, solo), g0 and g1 local to the recording.  A
//                       segmented scan and a compaction, nine short launches, no launch walks a run: a workgroup of SM_NT = 256 threads
//                       takes SM_SPAN = 2048 consecutive packed frames, 8 a thread, every scan is (thread, wave by __shfl_up, the 4 waves
//                       through LDS) and the per-workgroup totals are scanned by one workgroup in a launch of its own, so nothing depends on
//                       the order in which workgroups finish.
//                         1 classify   kind [G]: -1 silent, -2 overlapped, k solo for k; per workgroup the last frame that is not silent
//                         2 scan       ... made exclusive over the workgroups (maximum)
//                         3 count      p(g), the last frame before g that is not silent (a maximum scan over the PACKED grid: the recording
//                                      is checked afterwards), hence brk(g) for every g that is not silent - p(g) missing, in another
//                                      recording, of another kind, overlapped, or g - p(g) - 1 > gap - and per workgroup the brk frames and
//                                      the solo frames
//                         4 scan       ... made exclusive (sums)
//                         5 groups     the frames that are not silent fall into groups that start at the brk frames.  Group j starts at its
//                                      brk frame, ends at p(the next brk frame) and holds solo_before(next) - solo_before(its own) solo
//                                      frames; a group whose frames are solo is a run of the rule.  The thread of brk frame j writes
//                                      start [j], solo_before [j] and end [j - 1]; the thread of the last frame closes the last group
//                         6 keep       per workgroup of 2048 groups the number with a solo kind and solo >= min_frames
//                         7 scan       ... made exclusive (sums); the total is N
//                         8 fill       the kept groups to their rows
//                         9 run_off    run_off [r] = the kept groups that start before frame_off [r] (a binary search per recording)
//   sdk_samples_score   E [W][d] fp32 -> per clip the leave-one-out cosine to its own speaker and the best cosine to another speaker of the
//                       recording, in float64.  Three launches: clip sums c [M][d] (a workgroup per clip, a thread per column, the windows
//                       in order), speaker sums m [S][d] (a workgroup per speaker, the speaker's clips in ascending order, found 256 at a
//                       time by ballot), scores (a workgroup per clip; the rivals are dealt to its 4 waves, lanes over columns).  Every sum
//                       has one owner and a fixed order and there is no floating-point atomic: two runs give the same bytes.
#include "common.hpp"
#include "packed_grid.hpp"

namespace {

constexpr int SM_MAX_SPK = 1024;             // hypothesis speakers per recording (words.MAX_WORD_SPEAKERS)
constexpr int SM_NT = 256;
constexpr int SM_IPT = 8;                    // frames (groups) per thread
constexpr int SM_SPAN = SM_NT * SM_IPT;      // frames (groups) per workgroup: 2048 (ops_score.SAMPLES_SCAN_SPAN)
constexpr int SM_SILENT = -1, SM_OVER = -2;
constexpr int SM_MAX_DIM = 512;              // diarize_host.MAX_ASSIGN_DIM

// exclusive prefix sum of v over the workgroup's 256 threads, and the total; sh holds 4 ints
__device__ __forceinline__ int sm_block_excl_sum(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < SM_NT / 64; ++i) {
    const int s = sh[i];
    if (i < w) base += s;
    total += s;
  }
  __syncthreads();
  return base + inc - v;
}

// the same for the maximum (nothing: -1)
__device__ __forceinline__ int sm_block_excl_max(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc = max(inc, t);
  }
  if (lane == 63) sh[w] = inc;
  const int before = __shfl_up(inc, 1, 64);
  __syncthreads();
  int base = -1;
  total = -1;
#pragma unroll
  for (int i = 0; i < SM_NT / 64; ++i) {
    const int s = sh[i];
    if (i < w) base = max(base, s);
    total = max(total, s);
  }
  __syncthreads();
  return lane ? max(base, before) : base;
}

__global__ __launch_bounds__(SM_NT) void sm_classify_kernel(const int32_t* __restrict__ speakers, const int32_t* __restrict__ frame_off,
                                                            const int32_t* __restrict__ cent_off, int R, int G, int32_t* __restrict__ kind,
                                                            int32_t* __restrict__ blk_last) {
  __shared__ int sh[SM_NT / 64];
  const int64_t f0 = (int64_t)blockIdx.x * SM_SPAN + (int64_t)threadIdx.x * SM_IPT;
  int last = -1;
  if (f0 < G) {
    int r = pg_find_group(frame_off, R, (int)f0);
    const int2* sp = reinterpret_cast<const int2*>(speakers);
#pragma unroll
    for (int i = 0; i < SM_IPT; ++i) {
      const int f = (int)f0 + i;
      if (f >= G) break;
      r = pg_next_group(frame_off, R, r, f);
      const int K = min(max(cent_off[r + 1] - cent_off[r], 0), SM_MAX_SPK);
      const int2 h = sp[f];
      const bool on0 = h.x >= 0 && h.x < K, on1 = h.y >= 0 && h.y < K;
      const int kd = on0 ? ((on1 && h.y != h.x) ? SM_OVER : h.x) : (on1 ? h.y : SM_SILENT);
      kind[f] = kd;
      if (kd != SM_SILENT) last = f;
    }
  }
  int total;
  (void)sm_block_excl_max(last, sh, total);
  if (threadIdx.x == 0) blk_last[blockIdx.x] = total;
}

// one workgroup: a [n] (and b [n], or NULL) -> their exclusive scans in place, the totals to tot [0], tot [1].  is_max: maxima (nothing: -1)
__global__ __launch_bounds__(SM_NT) void sm_scan_blocks_kernel(int32_t* __restrict__ a, int32_t* __restrict__ b, int n, int is_max,
                                                               int32_t* __restrict__ tot) {
  __shared__ int sh[SM_NT / 64];
  int carry_a = is_max ? -1 : 0, carry_b = 0;
  for (int base = 0; base < n; base += SM_NT) {
    const int i = base + threadIdx.x;
    const int va = i < n ? a[i] : (is_max ? -1 : 0);
    int ta;
    if (is_max) {
      const int ea = sm_block_excl_max(va, sh, ta);
      if (i < n) a[i] = max(carry_a, ea);
      carry_a = max(carry_a, ta);
    } else {
      const int ea = sm_block_excl_sum(va, sh, ta);
      if (i < n) a[i] = carry_a + ea;
      carry_a += ta;
    }
    if (b) {
      const int vb = i < n ? b[i] : 0;
      int tb;
      const int eb = sm_block_excl_sum(vb, sh, tb);
      if (i < n) b[i] = carry_b + eb;
      carry_b += tb;
    }
  }
  if (threadIdx.x == 0) {
    tot[0] = carry_a;
    if (b) tot[1] = carry_b;
  }
}

// launches 3 (FILL = false: blk_brk, blk_solo = the workgroup's counts) and 5 (FILL = true: they hold the exclusive scans)
template <bool FILL>
__global__ __launch_bounds__(SM_NT) void sm_groups_kernel(const int32_t* __restrict__ kind, const int32_t* __restrict__ frame_off, int R, int G, int gap,
                                                          const int32_t* __restrict__ blk_last, int32_t* __restrict__ blk_brk,
                                                          int32_t* __restrict__ blk_solo, int32_t* __restrict__ grp_start,
                                                          int32_t* __restrict__ grp_end, int32_t* __restrict__ grp_solo, int32_t* __restrict__ counts) {
  __shared__ int sh[SM_NT / 64];
  const int64_t f0w = (int64_t)blockIdx.x * SM_SPAN + (int64_t)threadIdx.x * SM_IPT;
  const int f0 = (int)min(f0w, (int64_t)G);
  int k[SM_IPT];
  int last = -1;
#pragma unroll
  for (int i = 0; i < SM_IPT; ++i) {
    k[i] = f0 + i < G ? kind[f0 + i] : SM_SILENT;
    if (k[i] != SM_SILENT) last = f0 + i;
  }
  int unused;
  const int before = max(sm_block_excl_max(last, sh, unused), blk_last[blockIdx.x]);   // the last frame before f0 that is not silent, else -1
  int p = before, pk = before >= 0 ? kind[before] : SM_SILENT;
  int r = f0 < G ? pg_find_group(frame_off, R, f0) : 0;
  int n_brk = 0, n_solo = 0;
  unsigned brk = 0;
#pragma unroll
  for (int i = 0; i < SM_IPT; ++i) {
    if (k[i] == SM_SILENT) continue;
    const int f = f0 + i;
    r = pg_next_group(frame_off, R, r, f);
    const bool b = p < frame_off[r] || pk != k[i] || k[i] == SM_OVER || f - p - 1 > gap;       // p == -1 is before every recording
    if (b) { brk |= 1u << i; ++n_brk; }
    if (k[i] >= 0) ++n_solo;
    p = f;
    pk = k[i];
  }
  if constexpr (!FILL) {
    int t_brk, t_solo;
    (void)sm_block_excl_sum(n_brk, sh, t_brk);
    (void)sm_block_excl_sum(n_solo, sh, t_solo);
    if (threadIdx.x == 0) { blk_brk[blockIdx.x] = t_brk; blk_solo[blockIdx.x] = t_solo; }
  } else {
    int t;
    int j = blk_brk[blockIdx.x] + sm_block_excl_sum(n_brk, sh, t);
    int s = blk_solo[blockIdx.x] + sm_block_excl_sum(n_solo, sh, t);
    p = before;
#pragma unroll
    for (int i = 0; i < SM_IPT; ++i) {
      if (k[i] == SM_SILENT) continue;
      if (brk & (1u << i)) {
        grp_start[j] = f0 + i;
        grp_solo[j] = s;
        if (j > 0) grp_end[j - 1] = p;                          // j > 0: a frame that is not silent stands before this one, p >= 0
        ++j;
      }
      if (k[i] >= 0) ++s;
      p = f0 + i;
    }
    if (f0 < G && f0 + SM_IPT >= G) {                           // the thread of the last frame closes the last group
      counts[0] = j;
      if (j > 0) grp_end[j - 1] = p;
      grp_solo[j] = s;
    }
  }
}

// launches 6 (FILL = false) and 8 (FILL = true: blk_keep holds the exclusive scan)
template <bool FILL>
__global__ __launch_bounds__(SM_NT) void sm_keep_kernel(const int32_t* __restrict__ kind, const int32_t* __restrict__ grp_start,
                                                        const int32_t* __restrict__ grp_end, const int32_t* __restrict__ grp_solo,
                                                        const int32_t* __restrict__ counts, int min_frames, int32_t* __restrict__ blk_keep,
                                                        const int32_t* __restrict__ frame_off, int R, int32_t* __restrict__ rows, int rows_cap,
                                                        int32_t* __restrict__ kept_start) {
  __shared__ int sh[SM_NT / 64];
  const int J = counts[0];
  const int64_t j0 = (int64_t)blockIdx.x * SM_SPAN + (int64_t)threadIdx.x * SM_IPT;
  unsigned keep = 0;
  int n = 0;
#pragma unroll
  for (int i = 0; i < SM_IPT; ++i) {
    const int64_t j = j0 + i;
    if (j < J && kind[grp_start[j]] >= 0 && grp_solo[j + 1] - grp_solo[j] >= min_frames) { keep |= 1u << i; ++n; }
  }
  int total;
  const int before = sm_block_excl_sum(n, sh, total);
  if constexpr (!FILL) {
    if (threadIdx.x == 0) blk_keep[blockIdx.x] = total;
  } else {
    int idx = blk_keep[blockIdx.x] + before;
#pragma unroll
    for (int i = 0; i < SM_IPT; ++i) {
      if (!(keep & (1u << i))) continue;
      const int j = (int)j0 + i;
      if (idx < rows_cap) {
        const int g0 = grp_start[j], g1 = grp_end[j] + 1;
        const int base = frame_off[pg_find_group(frame_off, R, g0)];
        reinterpret_cast<int4*>(rows)[idx] = make_int4(kind[g0], g0 - base, g1 - base, grp_solo[j + 1] - grp_solo[j]);
        kept_start[idx] = g0;
      }
      ++idx;
    }
  }
}

__global__ __launch_bounds__(SM_NT) void sm_run_off_kernel(const int32_t* __restrict__ kept_start, const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ frame_off, int R, int rows_cap, int32_t* __restrict__ run_off) {
  const int r = blockIdx.x * SM_NT + threadIdx.x;
  if (r > R) return;
  const int N = min(counts[1], rows_cap), x = frame_off[r];
  int lo = 0, hi = N;                                           // the kept runs that start before frame_off[r]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kept_start[mid] < x) lo = mid + 1; else hi = mid;
  }
  run_off[r] = lo;
}

struct SmWs {                                                    // the workspace of sdk_samples_runs, in int32 elements
  size_t kind, grp_start, grp_end, grp_solo, kept_start, blk_last, blk_brk, blk_solo, blk_keep, counts, total;
  int nb;
};

SmWs sm_layout(int64_t G) {
  SmWs w;
  w.nb = (int)((G + SM_SPAN - 1) / SM_SPAN);
  const size_t g = (size_t)G, nb = (size_t)w.nb;
  w.kind = 0;
  w.grp_start = w.kind + g;
  w.grp_end = w.grp_start + g;
  w.grp_solo = w.grp_end + g;
  w.kept_start = w.grp_solo + g + 1;
  w.blk_last = w.kept_start + g;
  w.blk_brk = w.blk_last + nb;
  w.blk_solo = w.blk_brk + nb;
  w.blk_keep = w.blk_solo + nb;
  w.counts = w.blk_keep + nb;
  w.total = w.counts + 4;
  return w;
}

// ---------------------------------------------------------------------------------------------------------------- scores
constexpr int SS_NT = 256;

__global__ void ss_clip_sum_kernel(const float* __restrict__ E, const int32_t* __restrict__ clip_off, int W, int d, double* __restrict__ c,
                                   int32_t* __restrict__ out_i) {
  const int i = blockIdx.x;
  const int a = min(max(clip_off[i], 0), W), b = min(max(clip_off[i + 1], a), W);
  for (int j = threadIdx.x; j < d; j += blockDim.x) {
    double s = 0.0;
    for (int w = a; w < b; ++w) s += (double)E[(int64_t)w * d + j];
    c[(int64_t)i * d + j] = s;
  }
  if (threadIdx.x == 0) out_i[3 * (int64_t)i + 1] = b - a;
}

__global__ __launch_bounds__(SS_NT) void ss_speaker_sum_kernel(const double* __restrict__ c, const int32_t* __restrict__ clip_spk,
                                                               const int32_t* __restrict__ out_i, int M, int d, double* __restrict__ msum,
                                                               double* __restrict__ mean) {
  __shared__ unsigned long long masks[SS_NT / 64];
  const int s = blockIdx.x, tid = threadIdx.x;
  double acc[SM_MAX_DIM / SS_NT] = {0.0, 0.0};
  int64_t n_win = 0;
  for (int base = 0; base < M; base += SS_NT) {
    const int i = base + tid;
    const unsigned long long hit = __ballot(i < M && clip_spk[i] == s);
    if ((tid & 63) == 0) masks[tid >> 6] = hit;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SS_NT / 64; ++w) {
      unsigned long long m = masks[w];
      while (m) {                                               // the speaker's clips of this batch, ascending; uniform over the workgroup
        const int ii = base + 64 * w + __ffsll((long long)m) - 1;
        m &= m - 1;
        n_win += out_i[3 * (int64_t)ii + 1];
#pragma unroll
        for (int q = 0; q < SM_MAX_DIM / SS_NT; ++q) {
          const int col = tid + SS_NT * q;
          if (col < d) acc[q] += c[(int64_t)ii * d + col];
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < SM_MAX_DIM / SS_NT; ++q) {
    const int col = tid + SS_NT * q;
    if (col < d) {
      msum[(int64_t)s * d + col] = acc[q];
      mean[(int64_t)s * d + col] = n_win > 0 ? acc[q] / (double)n_win : 0.0;
    }
  }
}

__global__ __launch_bounds__(SS_NT) void ss_score_kernel(const double* __restrict__ c, const double* __restrict__ msum, const int32_t* __restrict__ clip_spk,
                                                         const int32_t* __restrict__ spk_off, int R, int S, int d, double* __restrict__ out_f,
                                                         int32_t* __restrict__ out_i) {
  __shared__ double red[SS_NT / 64][3];
  __shared__ double best_c[SS_NT / 64];
  __shared__ int best_t[SS_NT / 64];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = clip_spk[i];
  if (s < 0 || s >= S) {                                        // a clip of nobody: no score
    if (tid == 0) { out_f[2 * (int64_t)i] = 0.0; out_f[2 * (int64_t)i + 1] = 0.0; out_i[3 * (int64_t)i] = -1; out_i[3 * (int64_t)i + 2] = 1; }
    return;
  }
  const double* ci = c + (int64_t)i * d;
  const double* ms = msum + (int64_t)s * d;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  for (int col = tid; col < d; col += SS_NT) {
    const double a = ci[col], m = ms[col] - a;
    p0 += a * m; p1 += a * a; p2 += m * m;
  }
  p0 = wave_sum(p0); p1 = wave_sum(p1); p2 = wave_sum(p2);
  if (lane == 0) { red[w][0] = p0; red[w][1] = p1; red[w][2] = p2; }
  __syncthreads();
  p0 = p1 = p2 = 0.0;
#pragma unroll
  for (int x = 0; x < SS_NT / 64; ++x) { p0 += red[x][0]; p1 += red[x][1]; p2 += red[x][2]; }
  const bool alone = !(p1 > 0.0) || !(p2 > 0.0);
  const double own = alone ? 0.0 : p0 / (sqrt(p1) * sqrt(p2));
  // the rivals: the other speakers of the recording, dealt to the waves; the lanes hold the clip's columns lane, lane + 64, ..
  const int r = pg_find_group(spk_off, R, s);
  const int t0 = min(max(spk_off[r], 0), S), t1 = min(max(spk_off[r + 1], t0), S);
  double av[SM_MAX_DIM / 64];
#pragma unroll
  for (int q = 0; q < SM_MAX_DIM / 64; ++q) av[q] = lane + 64 * q < d ? ci[lane + 64 * q] : 0.0;
  double bc = 0.0;
  int bt = -1;
  if (p1 > 0.0) {
    for (int t = t0 + w; t < t1; t += SS_NT / 64) {
      if (t == s) continue;
      const double* mt = msum + (int64_t)t * d;
      double q0 = 0.0, q1 = 0.0;
#pragma unroll
      for (int q = 0; q < SM_MAX_DIM / 64; ++q) {
        if (lane + 64 * q < d) {
          const double m = mt[lane + 64 * q];
          q0 += av[q] * m; q1 += m * m;
        }
      }
      q0 = wave_sum(q0); q1 = wave_sum(q1);
      if (!(q1 > 0.0)) continue;
      const double cs = q0 / (sqrt(p1) * sqrt(q1));
      if (cs == cs && (bt < 0 || cs > bc)) { bc = cs; bt = t; }   // t ascends: at equal values the lower t stays
    }
  }
  if (lane == 0) { best_c[w] = bc; best_t[w] = bt; }
  __syncthreads();
  if (tid == 0) {
    bc = 0.0; bt = -1;
#pragma unroll
    for (int x = 0; x < SS_NT / 64; ++x) {
      const int t = best_t[x];
      if (t >= 0 && (bt < 0 || best_c[x] > bc || (best_c[x] == bc && t < bt))) { bc = best_c[x]; bt = t; }
    }
    out_f[2 * (int64_t)i] = own;
    out_f[2 * (int64_t)i + 1] = bt >= 0 ? bc : 0.0;
    out_i[3 * (int64_t)i] = bt >= 0 ? bt - t0 : -1;
    out_i[3 * (int64_t)i + 2] = alone ? 1 : 0;
  }
}

// one block: c [M][d] clip sums, then msum [S][d] speaker sums, then 256 bytes
size_t ss_carve(WsCarver c, int M, int S, int d, double** sums) {
  *sums = c.take<double>(((size_t)M + (size_t)S) * d + 256 / sizeof(double));
  return c.bytes();
}

}  // namespace

extern "C" size_t sdk_samples_runs_workspace_bytes(int64_t G) {
  if (!(G >= 0 && G < (1ll << 30))) {
    sdk_set_error("sdk_samples_runs_workspace_bytes: G=%lld (fewer than 2^30 frames)", (long long)G);
    return 0;
  }
  WsCarver c{};
  c.take<int32_t>(sm_layout(G).total);
  return c.bytes();
}

extern "C" int sdk_samples_runs(sdk_ctx* ctx, const int32_t* speakers, const int32_t* frame_off, const int32_t* cent_off, int R, int64_t G,
                                int max_hyp, int gap_frames, int min_frames, int32_t* run_off, int32_t* rows, int64_t rows_cap, void* ws, size_t ws_bytes,
                                void* stream) {
  SDK_REQUIRE(ctx, "sdk_samples_runs: null context");
  SDK_REQUIRE(R >= 1 && R < (1 << 28) && G >= 0 && G < (1ll << 30), "sdk_samples_runs: R=%d G=%lld (R at least 1, fewer than 2^30 frames)", R, (long long)G);
  SDK_REQUIRE(max_hyp >= 0 && max_hyp <= SM_MAX_SPK, "sdk_samples_runs: %d hypothesis speakers in a recording (at most %d)", max_hyp, SM_MAX_SPK);
  SDK_REQUIRE(gap_frames >= 0 && gap_frames < (1 << 30), "sdk_samples_runs: gap_frames=%d (0 .. 2^30 - 1)", gap_frames);
  SDK_REQUIRE(min_frames >= 1 && min_frames < (1 << 30), "sdk_samples_runs: min_frames=%d (1 .. 2^30 - 1)", min_frames);
  SDK_REQUIRE(rows_cap >= G / min_frames && rows_cap < (1ll << 30), "sdk_samples_runs: rows_cap=%lld (at least G / min_frames = %lld: the most runs %lld frames hold)",
              (long long)rows_cap, (long long)(G / min_frames), (long long)G);
  SDK_REQUIRE(frame_off && cent_off && run_off && (G == 0 || speakers) && (rows_cap == 0 || rows), "sdk_samples_runs: null argument");
  hipStream_t st = (hipStream_t)stream;
  if (G == 0) {
    SDK_HIP_OK(hipMemsetAsync(run_off, 0, (size_t)(R + 1) * sizeof(int32_t), st));
    return 0;
  }
  SDK_REQUIRE_WS("sdk_samples_runs", "sdk_samples_runs_workspace_bytes", ws, ws_bytes, sdk_samples_runs_workspace_bytes(G), 16);
  SDK_REQUIRE(((uintptr_t)rows & 15) == 0, "sdk_samples_runs: rows=%p must be 16-byte aligned", (void*)rows);
  const SmWs L = sm_layout(G);
  WsCarver carve{static_cast<char*>(ws), 0};
  int32_t* base = carve.take<int32_t>(L.total);                    // one block: sm_layout's offsets are inside it
  int32_t *kind = base + L.kind, *grp_start = base + L.grp_start, *grp_end = base + L.grp_end, *grp_solo = base + L.grp_solo;
  int32_t *kept_start = base + L.kept_start, *blk_last = base + L.blk_last, *blk_brk = base + L.blk_brk, *blk_solo = base + L.blk_solo;
  int32_t *blk_keep = base + L.blk_keep, *counts = base + L.counts;
  const dim3 grid((unsigned)L.nb), nt(SM_NT);
  const int g = (int)G, cap = (int)rows_cap;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 8.0 * G + 3 * 4.0 * G + 5 * 4.0 * G);
  hipLaunchKernelGGL(sm_classify_kernel, grid, nt, 0, st, speakers, frame_off, cent_off, R, g, kind, blk_last);
  hipLaunchKernelGGL(sm_scan_blocks_kernel, dim3(1), nt, 0, st, blk_last, (int32_t*)nullptr, L.nb, 1, counts + 2);
  hipLaunchKernelGGL(sm_groups_kernel<false>, grid, nt, 0, st, kind, frame_off, R, g, gap_frames, blk_last, blk_brk, blk_solo, grp_start, grp_end, grp_solo, counts);
  hipLaunchKernelGGL(sm_scan_blocks_kernel, dim3(1), nt, 0, st, blk_brk, blk_solo, L.nb, 0, counts + 2);
  hipLaunchKernelGGL(sm_groups_kernel<true>, grid, nt, 0, st, kind, frame_off, R, g, gap_frames, blk_last, blk_brk, blk_solo, grp_start, grp_end, grp_solo, counts);
  hipLaunchKernelGGL(sm_keep_kernel<false>, grid, nt, 0, st, kind, grp_start, grp_end, grp_solo, counts, min_frames, blk_keep, frame_off, R, rows, cap, kept_start);
  hipLaunchKernelGGL(sm_scan_blocks_kernel, dim3(1), nt, 0, st, blk_keep, (int32_t*)nullptr, L.nb, 0, counts + 1);
  hipLaunchKernelGGL(sm_keep_kernel<true>, grid, nt, 0, st, kind, grp_start, grp_end, grp_solo, counts, min_frames, blk_keep, frame_off, R, rows, cap, kept_start);
  hipLaunchKernelGGL(sm_run_off_kernel, dim3((unsigned)(R / SM_NT + 1)), nt, 0, st, kept_start, counts, frame_off, R, cap, run_off);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t sdk_samples_score_workspace_bytes(int M, int S, int d) {
  if (!(M >= 0 && M < (1 << 24) && S >= 0 && S < (1 << 24) && d >= 64 && d <= SM_MAX_DIM && d % 64 == 0)) {
    sdk_set_error("sdk_samples_score_workspace_bytes: M=%d S=%d d=%d (fewer than 2^24 clips and speakers, d a multiple of 64, at most %d)", M, S, d, SM_MAX_DIM);
    return 0;
  }
  double* sums;
  return ss_carve({}, M, S, d, &sums);
}

extern "C" int sdk_samples_score(sdk_ctx* ctx, const float* E, int W, int d, const int32_t* clip_off, const int32_t* clip_spk, int M,
                                 const int32_t* spk_off, int R, int S, double* mean, double* out_f, int32_t* out_i, void* ws, size_t ws_bytes,
                                 void* stream) {
  SDK_REQUIRE(ctx, "sdk_samples_score: null context");
  SDK_REQUIRE(d >= 64 && d <= SM_MAX_DIM && d % 64 == 0, "sdk_samples_score: d=%d not supported (a multiple of 64, at most %d)", d, SM_MAX_DIM);
  SDK_REQUIRE(W >= 0 && W < (1 << 24) && M >= 0 && M < (1 << 24) && R >= 1 && S >= 0 && S < (1 << 24),
              "sdk_samples_score: W=%d M=%d R=%d S=%d (fewer than 2^24 windows, clips and speakers, R at least 1)", W, M, R, S);
  SDK_REQUIRE(clip_off && spk_off && (W == 0 || E) && (M == 0 || (clip_spk && out_f && out_i)) && (S == 0 || mean), "sdk_samples_score: null argument");
  if (M == 0 && S == 0) return 0;
  SDK_REQUIRE_WS("sdk_samples_score", "sdk_samples_score_workspace_bytes", ws, ws_bytes, sdk_samples_score_workspace_bytes(M, S, d), 8);
  hipStream_t st = (hipStream_t)stream;
  double* c;
  ss_carve({static_cast<char*>(ws), 0}, M, S, d, &c);
  double* msum = c + (size_t)M * d;
  ProfScope ps(ctx, stream, SDK_K_COPY, 2.0 * W * (double)d, 4.0 * W * (double)d + 24.0 * ((double)M + S) * d);
  if (M) hipLaunchKernelGGL(ss_clip_sum_kernel, dim3((unsigned)M), dim3((unsigned)min(d, SS_NT)), 0, st, E, clip_off, W, d, c, out_i);
  if (S) hipLaunchKernelGGL(ss_speaker_sum_kernel, dim3((unsigned)S), dim3(SS_NT), 0, st, c, clip_spk, out_i, M, d, msum, mean);
  if (M) hipLaunchKernelGGL(ss_score_kernel, dim3((unsigned)M), dim3(SS_NT), 0, st, c, msum, clip_spk, spk_off, R, S, d, out_f, out_i);
  SDK_LAUNCH_CHECK();
  return 0;
}
