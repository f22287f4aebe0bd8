// Scoring a diarization the DIHARD way (score.py): the evaluation map (UEM) and the tables of the Jaccard error rate, on the packed frame grid
// (packed_grid.hpp) and the prefix-sum tables of score.hip.
//
//   score_uem_kernel        thread = frame: the recording by binary search on frame_off, then a binary search of its merged UEM intervals
//                           [s0, s1) (sorted, disjoint); scored = 0 where no interval holds the frame's centre.
//   score_dur_clear_kernel  thread = (recording, lane): ref_frames and hyp_frames of the recording = 0.
//   score_durations_kernel  ref_mask, scored, speakers [G][2] -> per recording ref_frames [S_r] and hyp_frames [K_r], the scored frames in which
//                           a reference / hypothesis speaker is active.  score_cooccur_kernel's walk (pg_walk): a workgroup takes SJ_FRAMES
//                           consecutive packed frames and serves the recordings inside them one at a time.  A wave counts speaker i over its
//                           64 frames with one ballot and keeps the count on lane i; the waves meet in 64 + 64 counters in LDS, then one
//                           integer atomic add per non-zero counter.
//   score_jaccard_kernel    thread = cell of the co tables: the recording by binary search on co_off,
//                           q = floor(co * 2^30 / (ref_frames[i] + hyp_frames[j] - co)) in unsigned 64-bit, 0 where co == 0.
//
// sdk_score_map (score.hip) then runs on q as it stands.  Everything is integer arithmetic: stores of one value and integer adds do not depend
// on the order they land in, so every output is bit-identical run to run.  No kernel needs an ordering between workgroups of one launch:
// the launches follow each other in stream order.
#include "common.hpp"
#include "packed_grid.hpp"

namespace {

constexpr int SJ_NT = 256;
constexpr int SJ_FPT = 16;                   // frames per thread of score_durations_kernel
constexpr int SJ_FRAMES = SJ_NT * SJ_FPT;    // frames per workgroup
constexpr int SJ_SHIFT = 30;                 // q is the Jaccard index in units of 2^-30

__global__ __launch_bounds__(SJ_NT) void score_uem_kernel(const int32_t* __restrict__ uem, const int32_t* __restrict__ uem_off,
                                                          const int32_t* __restrict__ frame_off, int R, int G, uint8_t* __restrict__ scored) {
  const int g = blockIdx.x * SJ_NT + threadIdx.x;
  if (g >= G) return;
  const int r = pg_find_group(frame_off, R, g);
  const int64_t centre = (int64_t)PG_HOP * (g - frame_off[r]) + PG_FIRST;
  int lo = uem_off[r], hi = uem_off[r + 1];                     // the last interval of [lo, hi) with s0 <= centre, if there is one
  const int first = lo;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (uem[2 * (int64_t)mid] <= centre) lo = mid + 1; else hi = mid;
  }
  if (lo == first || centre >= uem[2 * (int64_t)(lo - 1) + 1]) scored[g] = 0;
}

__global__ __launch_bounds__(SJ_NT) void score_dur_clear_kernel(const int32_t* __restrict__ ref_off, const int32_t* __restrict__ cent_off, int R,
                                                                int32_t* __restrict__ ref_frames, int32_t* __restrict__ hyp_frames) {
  const int t = blockIdx.x * SJ_NT + threadIdx.x;
  const int r = t >> 6, lane = t & 63;
  if (r >= R) return;
  if (lane < ref_off[r + 1] - ref_off[r]) ref_frames[ref_off[r] + lane] = 0;
  if (lane < cent_off[r + 1] - cent_off[r]) hyp_frames[cent_off[r] + lane] = 0;
}

__global__ __launch_bounds__(SJ_NT) void score_durations_kernel(const unsigned long long* __restrict__ ref_mask, const uint8_t* __restrict__ scored,
                                                                const int32_t* __restrict__ speakers, const int32_t* __restrict__ frame_off,
                                                                const int32_t* __restrict__ ref_off, const int32_t* __restrict__ cent_off, int R,
                                                                int G, int32_t* __restrict__ ref_frames, int32_t* __restrict__ hyp_frames) {
  __shared__ int32_t cnt[2 * PG_MAX_SPK];                       // [0, 64): reference speakers, [64, 128): hypothesis speakers
  const int tid = threadIdx.x, lane = tid & 63;
  const int f0 = blockIdx.x * SJ_FRAMES;
  pg_walk(frame_off, R, f0, min(f0 + SJ_FRAMES, G), [&](int r, int a, int b) {
    // not pg_speakers: a count below 0 already reads as none here, and its lower clamp cost this launch 1.4 %
    const int S = min(ref_off[r + 1] - ref_off[r], PG_MAX_SPK), K = min(cent_off[r + 1] - cent_off[r], PG_MAX_SPK);
    if (tid < 2 * PG_MAX_SPK) cnt[tid] = 0;
    __syncthreads();
    int n_ref = 0, n_hyp = 0;                                   // lane i: the wave's frames with reference / hypothesis speaker i
    for (int base = a; base < b; base += SJ_NT) {               // uniform bounds: the whole wave reaches every ballot
      const int g = base + tid;
      unsigned long long m = 0;
      int h0 = -1, h1 = -1;
      if (g < b && scored[g]) {
        m = ref_mask[g];
        h0 = speakers[2 * (int64_t)g];
        h1 = speakers[2 * (int64_t)g + 1];
      }
      for (int i = 0; i < S; ++i) {
        const int n = __popcll(__ballot((m >> i) & 1));
        if (lane == i) n_ref += n;
      }
      for (int j = 0; j < K; ++j) {                             // a name >= K or < 0 matches no j; named twice counts once
        const int n = __popcll(__ballot(h0 == j || h1 == j));
        if (lane == j) n_hyp += n;
      }
    }
    if (n_ref) atomicAdd(&cnt[lane], n_ref);
    if (n_hyp) atomicAdd(&cnt[PG_MAX_SPK + lane], n_hyp);
    __syncthreads();
    if (tid < S && cnt[tid]) atomicAdd(ref_frames + ref_off[r] + tid, cnt[tid]);
    if (tid >= PG_MAX_SPK && tid < PG_MAX_SPK + K && cnt[tid]) atomicAdd(hyp_frames + cent_off[r] + (tid - PG_MAX_SPK), cnt[tid]);
    __syncthreads();                                            // the counters are cleared again for the next recording
  });
}

__global__ __launch_bounds__(SJ_NT) void score_jaccard_kernel(const int32_t* __restrict__ co, const int32_t* __restrict__ ref_frames,
                                                              const int32_t* __restrict__ hyp_frames, const int32_t* __restrict__ ref_off,
                                                              const int32_t* __restrict__ cent_off, const int64_t* __restrict__ co_off, int R,
                                                              int64_t co_total, int32_t* __restrict__ q) {
  const int64_t c = (int64_t)blockIdx.x * SJ_NT + threadIdx.x;
  if (c >= co_total) return;
  const int32_t v = co[c];
  int32_t out = 0;
  if (v > 0) {
    const int r = pg_find_group(co_off, R, c);
    const int K = cent_off[r + 1] - cent_off[r];                // the recording holds cell c: S_r K_r > 0
    const int64_t cell = c - co_off[r];
    const int i = (int)(cell / K), j = (int)(cell % K);
    const unsigned long long den = (unsigned long long)(uint32_t)ref_frames[ref_off[r] + i] + (uint32_t)hyp_frames[cent_off[r] + j] - (uint32_t)v;
    // co <= ref_frames and co <= hyp_frames make den >= co, so the quotient is at most 2^30; tables that break this give 0 or the low 32 bits
    out = den ? (int32_t)(((unsigned long long)v << SJ_SHIFT) / den) : 0;
  }
  q[c] = out;
}

}  // namespace

extern "C" int sdk_score_uem(sdk_ctx* ctx, const int32_t* uem, const int32_t* uem_off, const int32_t* frame_off, int R, int U, int64_t G,
                             uint8_t* scored, void* stream) {
  SDK_REQUIRE(ctx, "sdk_score_uem: null context");
  SDK_REQUIRE(R >= 1 && U >= 0 && U < (1 << 28) && G >= 0 && G < (1ll << 30), "sdk_score_uem: R=%d U=%d G=%lld (R at least 1, fewer than 2^28 intervals and 2^30 frames)",
              R, U, (long long)G);
  if (G == 0) return 0;
  SDK_REQUIRE(scored && (U == 0 || (uem && uem_off && frame_off)), "sdk_score_uem: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 2.0 * G + 8.0 * U);
  if (U == 0) {                                                 // no interval anywhere: nothing is scored
    SDK_HIP_OK(hipMemsetAsync(scored, 0, (size_t)G, s));
    return 0;
  }
  hipLaunchKernelGGL(score_uem_kernel, pg_grid(G, SJ_NT), dim3(SJ_NT), 0, s, uem, uem_off, frame_off, R, (int)G, scored);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_score_durations(sdk_ctx* ctx, const uint64_t* ref_mask, const uint8_t* scored, const int32_t* speakers, const int32_t* frame_off,
                                   const int32_t* ref_off, const int32_t* cent_off, int R, int64_t G, int max_ref, int max_hyp,
                                   int32_t* ref_frames, int32_t* hyp_frames, void* stream) {
  SDK_REQUIRE(ctx, "sdk_score_durations: null context");
  SDK_REQUIRE(R >= 1 && R < (1 << 24) && G >= 0 && G < (1ll << 30), "sdk_score_durations: R=%d G=%lld (1 .. 2^24 - 1 recordings, fewer than 2^30 frames)", R, (long long)G);
  SDK_REQUIRE(max_ref >= 0 && max_ref <= PG_MAX_SPK && max_hyp >= 0 && max_hyp <= PG_MAX_SPK,
              "sdk_score_durations: %d reference and %d hypothesis speakers in a recording (at most %d each)", max_ref, max_hyp, PG_MAX_SPK);
  SDK_REQUIRE(ref_off && cent_off && (max_ref == 0 || ref_frames) && (max_hyp == 0 || hyp_frames), "sdk_score_durations: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 17.0 * G + 4.0 * R * (max_ref + max_hyp));
  if (max_ref || max_hyp) {
    hipLaunchKernelGGL(score_dur_clear_kernel, pg_grid((int64_t)R * 64, SJ_NT), dim3(SJ_NT), 0, s, ref_off, cent_off, R, ref_frames, hyp_frames);
    SDK_LAUNCH_CHECK();
  }
  if (G == 0 || (max_ref == 0 && max_hyp == 0)) return 0;
  SDK_REQUIRE(ref_mask && scored && speakers && frame_off, "sdk_score_durations: null argument");
  hipLaunchKernelGGL(score_durations_kernel, pg_grid(G, SJ_FRAMES), dim3(SJ_NT), 0, s, (const unsigned long long*)ref_mask, scored, speakers, frame_off, ref_off,
                     cent_off, R, (int)G, ref_frames, hyp_frames);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_score_jaccard(sdk_ctx* ctx, const int32_t* co, const int32_t* ref_frames, const int32_t* hyp_frames, const int32_t* ref_off,
                                 const int32_t* cent_off, const int64_t* co_off, int R, int64_t co_total, int32_t* q, void* stream) {
  SDK_REQUIRE(ctx, "sdk_score_jaccard: null context");
  SDK_REQUIRE(R >= 1 && co_total >= 0 && co_total <= (int64_t)R * PG_MAX_SPK * PG_MAX_SPK, "sdk_score_jaccard: R=%d co_total=%lld (R at least 1, at most %d x %d cells a recording)",
              R, (long long)co_total, PG_MAX_SPK, PG_MAX_SPK);
  if (co_total == 0) return 0;
  SDK_REQUIRE(co && ref_frames && hyp_frames && ref_off && cent_off && co_off && q, "sdk_score_jaccard: null argument");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 16.0 * co_total);
  hipLaunchKernelGGL(score_jaccard_kernel, pg_grid(co_total, SJ_NT), dim3(SJ_NT), 0, (hipStream_t)stream, co, ref_frames, hyp_frames, ref_off, cent_off, co_off, R,
                     co_total, q);
  SDK_LAUNCH_CHECK();
  return 0;
}
