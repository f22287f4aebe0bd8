// Speaker-attributed transcripts (words.py): the words of a transcript onto the per-frame speakers of a diarization, and the word-level
// diarization error rate (WDER) tables, on the packed frame grid (packed_grid.hpp).
//
//   words_attribute_kernel   words [W][2] (s0, s1 in samples of the word's recording), speakers [G][2] -> rows [W][8] int32 (speaker, votes,
//                            solo, span, second, second_votes, distance, g0).  One wave per word (a workgroup is one wave): the word's
//                            recording by binary search on word_off, its frames 64 at a time, one integer LDS atomic per speaker a frame
//                            names; the counters v[k] and u[k] of the recording's K_r <= 1024 speakers live in LDS (2 x cap int32 per wave,
//                            cap = the pack's largest K_r rounded up to 64).  The winner is a cross-lane maximum in the order (v descending,
//                            u descending, k ascending), taken twice (the second time without the winner); a word in non-speech searches its
//                            nearest voiced frame on both sides, 64 distances at a time.
//   words_cooccur_kernel     rows, ref [W] -> per recording co [S_r][K_r] int32 and tally [3] int64 (scored, unassigned, words).  A workgroup
//                            takes WD_WORDS consecutive words and serves the recordings inside them one at a time (pg_walk): the recording's
//                            table is summed in LDS (at most 64 x 64 int32), then one integer atomic add per non-zero cell
//                            (score_cooccur_kernel on words).  sdk_score_map then runs on co unchanged.
//
// Integer arithmetic only.  Integer adds do not depend on the order they land in and every row is written by one wave, so every output is
// bit-identical run to run.
#include "common.hpp"
#include "packed_grid.hpp"

namespace {

constexpr int WD_MAX_SPK = 1024;             // hypothesis speakers per recording (words.MAX_WORD_SPEAKERS); the WDER tables: PG_MAX_SPK a side
constexpr int WD_NT = 256;
constexpr int WD_WPT = 4;                    // words per thread of words_cooccur_kernel
constexpr int WD_WORDS = WD_NT * WD_WPT;     // words per workgroup
constexpr int WD_HALF = PG_FIRST - PG_HOP / 2;   // floor((m - WD_HALF) / PG_HOP): the frame whose centre is nearest m (half way: the later)

struct WdBest { int v, u, k; };              // k == -1: nobody

__device__ __forceinline__ bool wd_before(int v, int u, int k, const WdBest& b) {   // (v, u, k) stands before b in the order
  if (b.k < 0) return true;
  if (v != b.v) return v > b.v;
  if (u != b.u) return u > b.u;
  return k < b.k;
}

__device__ __forceinline__ WdBest wd_wave_best(WdBest b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(b.v, o, 64), ou = __shfl_xor(b.u, o, 64), ok = __shfl_xor(b.k, o, 64);
    if (ok >= 0 && wd_before(ov, ou, ok, b)) b = {ov, ou, ok};
  }
  return b;
}

// the first of the lanes' candidates in the order among the k < K with v[k] > 0, k != skip
__device__ __forceinline__ WdBest wd_scan(const int32_t* v, const int32_t* u, int K, int lane, int skip) {
  WdBest b = {0, 0, -1};
  for (int k = lane; k < K; k += 64) {
    const int vk = v[k], uk = u[k];
    if (vk > 0 && k != skip && wd_before(vk, uk, k, b)) b = {vk, uk, k};
  }
  return wd_wave_best(b);
}

// the first entry of packed frame f that names one of the K speakers, else -1
__device__ __forceinline__ int wd_named(const int32_t* __restrict__ speakers, int64_t f, int K) {
  const int h0 = speakers[2 * f], h1 = speakers[2 * f + 1];
  if (h0 >= 0 && h0 < K) return h0;
  if (h1 >= 0 && h1 < K) return h1;
  return -1;
}

__global__ __launch_bounds__(64) void words_attribute_kernel(const int32_t* __restrict__ words, const int32_t* __restrict__ word_off,
                                                             const int32_t* __restrict__ speakers, const int32_t* __restrict__ frame_off,
                                                             const int32_t* __restrict__ cent_off, int R, int W, int cap, int gap,
                                                             int32_t* __restrict__ out) {
  extern __shared__ int32_t wd_cnt[];                           // v[cap], u[cap]
  int32_t* v = wd_cnt;
  int32_t* u = wd_cnt + cap;
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= W) return;
  int32_t* row = out + 8 * (int64_t)w;
  const int r = pg_find_group(word_off, R, w);
  const int64_t fbase = frame_off[r];
  const int64_t n_g = frame_off[r + 1] - fbase;
  const int K = min(max(cent_off[r + 1] - cent_off[r], 0), cap);  // never past the counters, whatever the tables say
  if (n_g <= 0) {
    if (lane < 8) row[lane] = (lane == 0 || lane == 4 || lane == 6) ? -1 : 0;
    return;
  }
  const int64_t s0 = words[2 * (int64_t)w], s1 = words[2 * (int64_t)w + 1];
  int64_t g0 = min(pg_first_frame(s0), n_g), g1 = min(pg_first_frame(s1), n_g);
  if (g1 <= g0) {                                               // no centre inside [s0, s1): the frame nearest the midpoint
    const int64_t m = (s0 + s1) >> 1;
    const int64_t a = m - WD_HALF;
    g0 = min(a <= 0 ? (int64_t)0 : a / PG_HOP, n_g - 1);
    g1 = g0 + 1;
  }
  for (int k = lane; k < K; k += 64) { v[k] = 0; u[k] = 0; }
  __syncthreads();
  for (int64_t g = g0 + lane; g < g1; g += 64) {
    const int h0 = speakers[2 * (fbase + g)], h1 = speakers[2 * (fbase + g) + 1];
    const bool on0 = h0 >= 0 && h0 < K, on1 = h1 >= 0 && h1 < K && h1 != h0;
    if (on0) atomicAdd(&v[h0], 1);
    if (on1) atomicAdd(&v[h1], 1);
    if (on0 != on1) atomicAdd(&u[on0 ? h0 : h1], 1);
  }
  __syncthreads();
  const WdBest first = wd_scan(v, u, K, lane, -1);
  const int span = (int)(g1 - g0);
  if (first.k >= 0) {
    const WdBest second = wd_scan(v, u, K, lane, first.k);
    if (lane == 0) {
      row[0] = first.k; row[1] = first.v; row[2] = first.u; row[3] = span;
      row[4] = second.k; row[5] = second.k >= 0 ? second.v : 0; row[6] = 0; row[7] = (int)g0;
    }
    return;
  }
  // non-speech: the least delta in 1 .. gap with a voiced frame g0 - delta or g1 - 1 + delta inside the recording; the earlier side first
  int spk = -1, dist = -1;
  for (int64_t d0 = 1; d0 <= gap; d0 += 64) {
    if (g0 - d0 < 0 && g1 - 1 + d0 >= n_g) break;               // both sides have left the recording
    const int64_t d = d0 + lane;
    int cand = -1;
    if (d <= gap) {
      if (g0 - d >= 0) cand = wd_named(speakers, fbase + g0 - d, K);
      if (cand < 0 && g1 - 1 + d < n_g) cand = wd_named(speakers, fbase + g1 - 1 + d, K);
    }
    const unsigned long long hit = __ballot(cand >= 0);
    if (hit) {
      const int src = __ffsll((long long)hit) - 1;              // the least delta of this batch
      spk = __shfl(cand, src, 64);
      dist = (int)(d0 + src);
      break;
    }
  }
  if (lane == 0) {
    row[0] = spk; row[1] = 0; row[2] = 0; row[3] = span; row[4] = -1; row[5] = 0; row[6] = dist; row[7] = (int)g0;
  }
}

__global__ __launch_bounds__(WD_NT) void words_cooccur_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ ref,
                                                              const int32_t* __restrict__ word_off, const int32_t* __restrict__ ref_off,
                                                              const int32_t* __restrict__ cent_off, const int64_t* __restrict__ co_off, int R,
                                                              int W, int32_t* __restrict__ co, unsigned long long* __restrict__ tally) {
  __shared__ int32_t tab[PG_MAX_SPK * PG_MAX_SPK];
  __shared__ int32_t tal[3];
  const int tid = threadIdx.x;
  const int w0 = blockIdx.x * WD_WORDS;
  pg_walk(word_off, R, w0, min(w0 + WD_WORDS, W), [&](int r, int a, int b) {
    const int S = pg_speakers(ref_off, r), K = pg_speakers(cent_off, r);
    pg_co_clear<3, WD_NT>(tab, tal, S * K);
    int n_sc = 0, n_un = 0, n_w = 0;
    for (int x = a + tid; x < b; x += WD_NT) {
      const int i = ref[x], j = rows[8 * (int64_t)x];
      n_w += 1;
      if (i < 0 || i >= S) continue;                            // not scored
      n_sc += 1;
      if (j >= 0 && j < K) atomicAdd(&tab[i * K + j], 1); else n_un += 1;
    }
    pg_co_flush<3, WD_NT>(tab, tal, {n_sc, n_un, n_w}, S * K, co + co_off[r], tally + 3 * (int64_t)r);
  });
}

}  // namespace

extern "C" int sdk_words_attribute(sdk_ctx* ctx, const int32_t* words, const int32_t* word_off, const int32_t* speakers, const int32_t* frame_off,
                                   const int32_t* cent_off, int R, int W, int64_t G, int max_hyp, int gap_frames, int32_t* out, void* stream) {
  SDK_REQUIRE(ctx, "sdk_words_attribute: null context");
  SDK_REQUIRE(R >= 1 && W >= 0 && W < (1 << 28) && G >= 0 && G < (1ll << 30),
              "sdk_words_attribute: R=%d W=%d G=%lld (R at least 1, fewer than 2^28 words and 2^30 frames)", R, W, (long long)G);
  SDK_REQUIRE(max_hyp >= 0 && max_hyp <= WD_MAX_SPK, "sdk_words_attribute: %d hypothesis speakers in a recording (at most %d)", max_hyp, WD_MAX_SPK);
  SDK_REQUIRE(gap_frames >= 0 && gap_frames < (1 << 30), "sdk_words_attribute: gap_frames=%d (0 .. 2^30 - 1)", gap_frames);
  if (W == 0) return 0;
  SDK_REQUIRE(words && word_off && frame_off && cent_off && out && (G == 0 || speakers), "sdk_words_attribute: null argument");
  const int cap = max_hyp <= 64 ? 64 : (max_hyp + 63) / 64 * 64;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 40.0 * W + 8.0 * G);
  hipLaunchKernelGGL(words_attribute_kernel, dim3((unsigned)W), dim3(64), (size_t)cap * 8, (hipStream_t)stream, words, word_off, speakers, frame_off,
                     cent_off, R, W, cap, gap_frames, out);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_words_cooccur(sdk_ctx* ctx, const int32_t* rows, const int32_t* ref, const int32_t* word_off, const int32_t* ref_off,
                                 const int32_t* cent_off, const int64_t* co_off, int R, int W, int max_ref, int max_hyp, int64_t co_total, int32_t* co,
                                 int64_t* tally, void* stream) {
  SDK_REQUIRE(ctx, "sdk_words_cooccur: null context");
  SDK_REQUIRE(R >= 1 && W >= 0 && W < (1 << 28) && co_total >= 0, "sdk_words_cooccur: R=%d W=%d co_total=%lld (R at least 1, fewer than 2^28 words)", R, W,
              (long long)co_total);
  SDK_REQUIRE(max_ref >= 0 && max_ref <= PG_MAX_SPK && max_hyp >= 0 && max_hyp <= PG_MAX_SPK,
              "sdk_words_cooccur: %d reference and %d hypothesis speakers in a recording (at most %d each)", max_ref, max_hyp, PG_MAX_SPK);
  SDK_REQUIRE(tally && (co_total == 0 || co), "sdk_words_cooccur: null argument (co=%p tally=%p)", (void*)co, (void*)tally);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 8.0 * W + 4.0 * co_total);
  SDK_HIP_OK(hipMemsetAsync(tally, 0, (size_t)R * 3 * 8, s));
  if (co_total) SDK_HIP_OK(hipMemsetAsync(co, 0, (size_t)co_total * 4, s));
  if (W == 0) return 0;
  SDK_REQUIRE(rows && ref && word_off && ref_off && cent_off && co_off, "sdk_words_cooccur: null argument");
  hipLaunchKernelGGL(words_cooccur_kernel, pg_grid(W, WD_WORDS), dim3(WD_NT), 0, s, rows, ref, word_off, ref_off, cent_off, co_off,
                     R, W, co, (unsigned long long*)tally);
  SDK_LAUNCH_CHECK();
  return 0;
}
