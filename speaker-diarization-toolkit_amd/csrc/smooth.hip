// Smoothing of diarized turns (smooth.py): fill a speaker's short pauses, then drop the short runs, on the packed frame grid
// (packed_grid.hpp).  Integers only: every frame has one owner in every launch and the tallies are integer atomic sums, so two runs give the
// same bytes.  The kernels hold no per-speaker memory, so the cost does not depend on K_r.
//
//   sdk_smooth_turns    speakers [G][2] in and out, tallies [R][2] = (filled, dropped).  Three launches of one thread per frame, SMT_NT = 256
//                       frames a workgroup; a frame finds its recording by binary search on frame_off and no walk leaves the recording.
//                         1 next    ent [g] = (c0, c1, d0, d1): the frame's speakers in canonical form (an entry < 0 or >= K_r is -1, a speaker
//                                   named twice stands once, compacted to the low slot) and, per entry, d = the distance to the next frame
//                                   that names the same speaker, looked for over fill + 1 frames; 0: none.  An entry whose next frame names
//                                   the speaker again has d = 1 after one read: only the last frame of a run walks
//                         2 fill    frame g reads ent [g - j] for j = 1 .. fill: an entry there with d > j is the end of the one run whose gap
//                                   (of d - 1 <= fill frames) covers g, so every filler of g shows up exactly once and none is named by g.
//                                   The smallest cap - (the speakers g names) of them go behind g's own: mid [g].  A frame without a free
//                                   slot reads nothing
//                         3 drop    per entry of mid [g] the same speaker is counted over at most keep - 1 frames to each side, stopping
//                                   where the run ends or keep frames are known; an entry of a run shorter than keep is cleared, the frame
//                                   compacted and written back to speakers
//                       No launch writes what it reads of other frames: 1 reads speakers and writes ent, 2 reads ent and writes mid, 3 reads
//                       mid and writes speakers.  The walks of 2 and 3 read consecutive frames from consecutive lanes (coalesced, from the L2).
#include "common.hpp"
#include "packed_grid.hpp"

namespace {

constexpr int SMT_NT = 256;                  // frames per workgroup (smooth.SMOOTH_BLOCK_FRAMES)
constexpr int SMT_MAX_FRAMES = 1024;         // the longest fill and keep, in frames (smooth.MAX_SMOOTH_FRAMES)

// v added to tally [2 r + which]: one atomic per wave where the wave lies inside one recording (almost always), else one per lane
__device__ __forceinline__ void smt_tally(int32_t* __restrict__ tallies, int r, int which, int v, bool live) {
  const int r0 = __builtin_amdgcn_readfirstlane(r);
  if (__all(!live || r == r0)) {
    const int s = wave_sum(live ? v : 0);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tallies[2 * (int64_t)r0 + which], s);
  } else if (live && v) {
    atomicAdd(&tallies[2 * (int64_t)r + which], v);
  }
}

__global__ __launch_bounds__(SMT_NT) void smt_next_kernel(const int32_t* __restrict__ speakers, const int32_t* __restrict__ frame_off,
                                                          const int32_t* __restrict__ cent_off, int R, int G, int fill, int4* __restrict__ ent) {
  const int64_t gw = (int64_t)blockIdx.x * SMT_NT + threadIdx.x;
  if (gw >= G) return;
  const int g = (int)gw;
  const int r = pg_find_group(frame_off, R, g);
  const int end = min(frame_off[r + 1], G);
  const int K = max(cent_off[r + 1] - cent_off[r], 0);
  const int2* sp = reinterpret_cast<const int2*>(speakers);
  const int2 h = sp[g];
  const bool on0 = h.x >= 0 && h.x < K, on1 = h.y >= 0 && h.y < K && !(on0 && h.y == h.x);
  const int c0 = on0 ? h.x : (on1 ? h.y : -1), c1 = (on0 && on1) ? h.y : -1;
  int d0 = 0, d1 = 0;
  const int last = min(g + fill + 1, end - 1);                  // the frames of the recording within fill + 1 of g
  if (c0 >= 0) {
    for (int f = g + 1; f <= last; ++f) {
      const int2 n = sp[f];                                     // c0 is a speaker of this recording: a raw entry equal to it names it
      if (n.x == c0 || n.y == c0) { d0 = f - g; break; }
    }
  }
  if (c1 >= 0) {
    for (int f = g + 1; f <= last; ++f) {
      const int2 n = sp[f];
      if (n.x == c1 || n.y == c1) { d1 = f - g; break; }
    }
  }
  ent[g] = make_int4(c0, c1, d0, d1);
}

__global__ __launch_bounds__(SMT_NT) void smt_fill_kernel(const int4* __restrict__ ent, const int32_t* __restrict__ frame_off, int R, int G, int fill,
                                                          int cap, int2* __restrict__ mid, int32_t* __restrict__ tallies) {
  const int64_t gw = (int64_t)blockIdx.x * SMT_NT + threadIdx.x;
  const bool live = gw < G;
  int r = 0, added = 0;
  if (live) {
    const int g = (int)gw;
    r = pg_find_group(frame_off, R, g);
    const int start = max(frame_off[r], 0);
    const int4 e = ent[g];
    int o0 = e.x, o1 = e.y;
    const int room = cap - (o0 >= 0) - (o1 >= 0);               // cap = 1 and two speakers named: -1, nothing is removed
    if (room > 0) {
      constexpr int NONE = 0x7fffffff;
      int m0 = NONE, m1 = NONE;                                 // the two smallest fillers, m0 < m1 (every filler shows up once)
      const int reach = min(fill, g - start);
      for (int j = 1; j <= reach; ++j) {
        const int4 p = ent[g - j];
        if (p.z > j) { if (p.x < m0) { m1 = m0; m0 = p.x; } else if (p.x < m1) m1 = p.x; }
        if (p.w > j) { if (p.y < m0) { m1 = m0; m0 = p.y; } else if (p.y < m1) m1 = p.y; }
      }
      if (o0 < 0) {                                             // nobody named: room is cap
        if (m0 != NONE) { o0 = m0; ++added; }
        if (room > 1 && m1 != NONE) { o1 = m1; ++added; }
      } else if (m0 != NONE) {                                  // one named and cap = 2
        o1 = m0; ++added;
      }
    }
    mid[g] = make_int2(o0, o1);
  }
  smt_tally(tallies, r, 0, added, live);
}

// the frames of [start, end) around g that name k, counted outwards from g until the run ends or `need` more are known
__device__ __forceinline__ int smt_run_around(const int2* __restrict__ mid, int g, int start, int end, int k, int need) {
  int n = 0;
  for (int f = g - 1; f >= start && n < need; --f) {
    const int2 m = mid[f];
    if (m.x != k && m.y != k) break;
    ++n;
  }
  for (int f = g + 1; f < end && n < need; ++f) {
    const int2 m = mid[f];
    if (m.x != k && m.y != k) break;
    ++n;
  }
  return n;
}

__global__ __launch_bounds__(SMT_NT) void smt_drop_kernel(const int2* __restrict__ mid, const int32_t* __restrict__ frame_off, int R, int G, int keep,
                                                          int32_t* __restrict__ speakers, int32_t* __restrict__ tallies) {
  const int64_t gw = (int64_t)blockIdx.x * SMT_NT + threadIdx.x;
  const bool live = gw < G;
  int r = 0, dropped = 0;
  if (live) {
    const int g = (int)gw;
    r = pg_find_group(frame_off, R, g);
    const int start = max(frame_off[r], 0), end = min(frame_off[r + 1], G);
    const int2 m = mid[g];
    int o0 = m.x, o1 = m.y;
    if (keep > 1) {                                             // a run holds a frame at least: keep <= 1 removes nothing
      if (o0 >= 0 && smt_run_around(mid, g, start, end, o0, keep - 1) < keep - 1) { o0 = -1; ++dropped; }
      if (o1 >= 0 && smt_run_around(mid, g, start, end, o1, keep - 1) < keep - 1) { o1 = -1; ++dropped; }
      if (o0 < 0) { o0 = o1; o1 = -1; }
    }
    reinterpret_cast<int2*>(speakers)[g] = make_int2(o0, o1);
  }
  smt_tally(tallies, r, 1, dropped, live);
}

// one block: ent [G] int4, then mid [G] int2, then 256 bytes (never 0 bytes: that is the refusal)
size_t smt_carve(WsCarver c, int64_t G, int4** ent) {
  *ent = (int4*)c.take<char>((size_t)G * (sizeof(int4) + sizeof(int2)) + 256);
  return c.bytes();
}

}  // namespace

extern "C" size_t sdk_smooth_turns_workspace_bytes(int64_t G) {
  if (!(G >= 0 && G < (1ll << 30))) {
    sdk_set_error("sdk_smooth_turns_workspace_bytes: G=%lld (fewer than 2^30 frames)", (long long)G);
    return 0;
  }
  int4* ent;
  return smt_carve({}, G, &ent);
}

extern "C" int sdk_smooth_turns(sdk_ctx* ctx, int32_t* speakers, const int32_t* frame_off, const int32_t* cent_off, int R, int64_t G, int fill_frames,
                                int keep_frames, int cap, int32_t* tallies, void* ws, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx, "sdk_smooth_turns: null context");
  SDK_REQUIRE(R >= 1 && R < (1 << 28) && G >= 0 && G < (1ll << 30), "sdk_smooth_turns: R=%d G=%lld (R at least 1, fewer than 2^30 frames)", R, (long long)G);
  SDK_REQUIRE(fill_frames >= 0 && fill_frames <= SMT_MAX_FRAMES, "sdk_smooth_turns: fill_frames=%d (0 .. %d)", fill_frames, SMT_MAX_FRAMES);
  SDK_REQUIRE(keep_frames >= 0 && keep_frames <= SMT_MAX_FRAMES, "sdk_smooth_turns: keep_frames=%d (0 .. %d)", keep_frames, SMT_MAX_FRAMES);
  SDK_REQUIRE(cap == 1 || cap == 2, "sdk_smooth_turns: cap=%d (1 or 2 speakers per frame)", cap);
  SDK_REQUIRE(frame_off && cent_off && tallies && (G == 0 || speakers), "sdk_smooth_turns: null argument");
  hipStream_t st = (hipStream_t)stream;
  if (G > 0) {                                         // every refusal comes before the first write: a refused call leaves tallies as they were
    SDK_REQUIRE_WS("sdk_smooth_turns", "sdk_smooth_turns_workspace_bytes", ws, ws_bytes, sdk_smooth_turns_workspace_bytes(G), 16);
    SDK_REQUIRE(((uintptr_t)speakers & 7) == 0, "sdk_smooth_turns: speakers=%p must be 8-byte aligned", (void*)speakers);
  }
  SDK_HIP_OK(hipMemsetAsync(tallies, 0, (size_t)R * 2 * sizeof(int32_t), st));
  if (G == 0) return 0;
  int4* ent;
  smt_carve({static_cast<char*>(ws), 0}, G, &ent);
  int2* mid = reinterpret_cast<int2*>(ent + G);
  const dim3 grid = pg_grid(G, SMT_NT), nt(SMT_NT);
  const int g = (int)G;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (8.0 + 16.0) * G + (16.0 + 8.0) * G + (8.0 + 8.0) * G);
  hipLaunchKernelGGL(smt_next_kernel, grid, nt, 0, st, speakers, frame_off, cent_off, R, g, fill_frames, ent);
  hipLaunchKernelGGL(smt_fill_kernel, grid, nt, 0, st, ent, frame_off, R, g, fill_frames, cap, mid, tallies);
  hipLaunchKernelGGL(smt_drop_kernel, grid, nt, 0, st, mid, frame_off, R, g, keep_frames, speakers, tallies);
  SDK_LAUNCH_CHECK();
  return 0;
}
