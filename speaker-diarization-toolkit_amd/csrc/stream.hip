// Streaming diarization (stream.py): the back half of a bank step - everything after the embedding of the streams' due chunks.
//
//   stream_step_kernel       block = one stream.  The chunk's candidate rows go to LDS; wave 0 maps them onto the stream's speaker table (the
//                            constrained assignment of diarize_assign.hpp on the unit centroids, then match / found / keep per candidate in
//                            slot order); the block renews the (at most three) sums and unit centroids that changed; then every thread owns
//                            frames of the ring: it clears those that newly come into reach, adds the chunk's frame and emits the frame
//                            when its latency has passed.
//   stream_flush_kernel      the end of a stream: every frame not yet emitted, up to the recording's last.
//   stream_reset_kernel, stream_centroids_kernel
//
// The state block (per stream: StreamHdr, sums, unit centroids, ring) stays on the device; the host reads none of it to take a step.  One
// owner per output element and per state element, every float64 sum in a fixed order, no atomics: two runs agree bit for bit.  A stream whose
// active flag is 0 is not touched at all.
#include "common.hpp"
#include "diarize_assign.hpp"

namespace {

constexpr int ST_NT = 256;
constexpr int ST_RING = SDK_STREAM_RING;            // frames per stream; a power of two
constexpr int ST_MAXK = SDK_STREAM_MAX_SPEAKERS;
constexpr int ST_TRAIN_DEN = 5;                      // diarize.TRAIN_CLEAN_DEN: a long candidate has 5 * clean_frames >= F
static_assert((ST_RING & (ST_RING - 1)) == 0, "the ring is indexed by g & (ST_RING - 1)");

struct StreamHdr {
  int64_t frontier;                                  // the next frame to emit
  int64_t reach;                                     // frames below it have been cleared and may hold counts
  int32_t K;
  int32_t pad[3];
  int32_t n[ST_MAXK];                                // rows added to every speaker's sum
};
static_assert(sizeof(StreamHdr) % 16 == 0, "the sums behind the header are read as double2");

struct StreamLayout {
  int64_t per, sums, unit, nc, cnt, act;             // bytes: a stream's block and the offsets inside it
  int stride;                                        // uint16 per ring row of act: capacity rounded up to 8 (16-byte rows)
};

__host__ __device__ inline StreamLayout st_layout(int capacity, int d) {
  StreamLayout l;
  l.stride = (capacity + 7) & ~7;
  l.sums = (int64_t)sizeof(StreamHdr);
  l.unit = l.sums + (int64_t)capacity * d * 8;
  l.nc = l.unit + (int64_t)capacity * d * 8;
  l.cnt = l.nc + (int64_t)ST_RING * 2;
  l.act = l.cnt + (int64_t)ST_RING * 2;
  l.per = (l.act + (int64_t)ST_RING * l.stride * 2 + 255) & ~(int64_t)255;
  return l;
}

struct StreamView {
  StreamHdr* hdr;
  double* sums;
  double* unit;
  uint16_t* nc;
  uint16_t* cnt;
  uint16_t* act;
};

__device__ __forceinline__ StreamView st_view(void* state, const StreamLayout& l, int r) {
  char* p = (char*)state + (int64_t)r * l.per;
  return {(StreamHdr*)p, (double*)(p + l.sums), (double*)(p + l.unit), (uint16_t*)(p + l.nc), (uint16_t*)(p + l.cnt), (uint16_t*)(p + l.act)};
}

// one frame leaves the ring: the mean chunk count rounded half up and capped, and the speakers of largest act > 0, ties to the lower id
__device__ __forceinline__ void emit_frame(int nc, int cn, const uint16_t* __restrict__ a, int K, int cap2, uint8_t* __restrict__ count,
                                           int32_t* __restrict__ speakers) {
  int a1 = 0, k1 = -1, a2 = 0, k2 = -1;
  if (a)
    for (int k = 0; k < K; ++k) {
      const int v = a[k];
      if (v > a1) { a2 = a1; k2 = k1; a1 = v; k1 = k; }
      else if (v > a2) { a2 = v; k2 = k; }
    }
  int n = nc ? (2 * cn + nc) / (2 * nc) : 0;
  n = min(n, cap2);
  *count = (uint8_t)n;
  speakers[0] = n >= 1 ? k1 : -1;
  speakers[1] = n >= 2 ? k2 : -1;
}

__global__ __launch_bounds__(ST_NT) void stream_step_kernel(const float* __restrict__ E, const int32_t* __restrict__ info,
                                                            const uint8_t* __restrict__ cls, const int64_t* __restrict__ starts,
                                                            const uint8_t* __restrict__ active, const int64_t* __restrict__ n_end, int F, int d,
                                                            int capacity, int hold, double delta_new, int cap2, void* __restrict__ state, StreamLayout lay,
                                                            int32_t* __restrict__ labels, float* __restrict__ score, int32_t* __restrict__ Kout,
                                                            int64_t* __restrict__ emit_lo, int32_t* __restrict__ emit_n,
                                                            uint8_t* __restrict__ count, int32_t* __restrict__ speakers) {
  const int r = blockIdx.x, tid = threadIdx.x;
  if (!active[r]) return;                                // uniform over the block
  __shared__ AssignLds L;
  __shared__ int s_lab[3], s_how[3], s_K;                // s_how: 0 nothing, 1 the row joins s_lab's sum, 2 the row founds s_lab
  __shared__ double s_red[ST_NT / 64];
  const StreamView st = st_view(state, lay, r);
  const int K0 = st.hdr->K;
  const int64_t frontier = st.hdr->frontier, reach0 = st.hdr->reach;
  const int32_t* in = info + (int64_t)r * 12;
  bool cand[3], lng[3];
  assign_candidates(in, cand);
#pragma unroll
  for (int s = 0; s < 3; ++s) lng[s] = cand[s] && (int64_t)ST_TRAIN_DEN * in[s * 4 + 1] >= F;
  assign_stage(L, E + (int64_t)r * 3 * d, cand, d, tid, ST_NT);
  __syncthreads();

  // ---- the mapping: wave 0
  if (tid < 64) {
    int32_t lab[3] = {-1, -1, -1};
    double cosv[3] = {0.0, 0.0, 0.0};
    if (K0 > 0) assign_solve(L, cand, st.unit, K0, d, 1, tid, lab, cosv);
    if (tid == 0) {
      int K = K0;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        int how = 0;
        float sc = 0.f;
        if (!cand[s]) {
          lab[s] = -1;
        } else if (K0 == 0) {                            // an empty table: the long candidates found it, in slot order
          if (lng[s] && K < capacity) { lab[s] = K++; how = 2; sc = 1.f; }
          else lab[s] = -1;
        } else {
          const bool matched = lab[s] >= 0 && 1.0 - cosv[s] <= delta_new;
          sc = lab[s] >= 0 ? (float)cosv[s] : 0.f;       // the cosine to the centroid as it stood before the update
          if (lng[s] && matched) how = 1;
          else if (lng[s] && K < capacity) { lab[s] = K++; how = 2; sc = 1.f; }
        }
        s_lab[s] = lab[s];
        s_how[s] = how;
        labels[(int64_t)r * 3 + s] = lab[s];
        score[(int64_t)r * 3 + s] = sc;
      }
      s_K = K;
      Kout[r] = K;
    }
  }
  __syncthreads();
  const int K = s_K;

  // ---- the sums and unit centroids that changed: thread = the columns tid, tid + 256; a centroid takes at most one row per step
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int how = s_how[s];                            // uniform over the block
    if (!how) continue;
    const int k = s_lab[s];
    double* Sk = st.sums + (int64_t)k * d;
    double* Uk = st.unit + (int64_t)k * d;
    const int j0 = tid, j1 = tid + ST_NT;
    double v0 = 0.0, v1 = 0.0;
    if (j0 < d) v0 = (how == 1 ? Sk[j0] : 0.0) + L.e[s][j0];
    if (j1 < d) v1 = (how == 1 ? Sk[j1] : 0.0) + L.e[s][j1];
    const double nrm = fmax(sqrt(block_sum(v0 * v0 + v1 * v1, s_red)), 1e-300);
    if (j0 < d) { Sk[j0] = v0; Uk[j0] = v0 / nrm; }
    if (j1 < d) { Sk[j1] = v1; Uk[j1] = v1 / nrm; }
    if (tid == 0) st.hdr->n[k] = how == 1 ? st.hdr->n[k] + 1 : 1;
  }

  // ---- the ring: thread = frame.  The chunk reaches the frames below reach1; those from reach0 on are new and cleared first.
  const int64_t q = chunk_q(starts[r]);                  // frame g of the stream is frame g + q of the chunk
  const int64_t reach1 = (int64_t)F - q;
  int64_t lo = frontier;
  if (reach1 - lo > ST_RING) lo = reach1 - ST_RING;      // starts that leap ahead: the ring never holds more than its size
  int64_t front1 = max(frontier, reach1 - hold);
  if (n_end && n_end[r] > 0) front1 = max(frontier, min(front1, dz_frames(n_end[r])));   // the stream's last chunk: no frame beyond its end
  const int l0 = s_lab[0], l1 = s_lab[1], l2 = s_lab[2];
  const uint8_t* c = cls + (int64_t)r * F;
  for (int64_t g = lo + tid; g < reach1; g += ST_NT) {
    const int slot = (int)(g & (ST_RING - 1));
    const bool fresh = g >= reach0;
    const int64_t i = g + q;
    const bool inside = i >= 0 && i < F;
    const int m = inside ? cls_mask(c[i]) : 0;
    uint16_t* a = st.act + (int64_t)slot * lay.stride;
    int nc = fresh ? 0 : st.nc[slot], cn = fresh ? 0 : st.cnt[slot];
    if (fresh) {
      uint4* z = reinterpret_cast<uint4*>(a);
      for (int j = 0; j < lay.stride / 8; ++j) z[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (inside) {
      ++nc;
      cn += __popc(m);
      const bool on0 = (m & 1) && l0 >= 0, on1 = (m & 2) && l1 >= 0, on2 = (m & 4) && l2 >= 0;
      if (on0) a[l0] += 1;
      if (on1 && !(on0 && l1 == l0)) a[l1] += 1;         // act counts a chunk once per speaker
      if (on2 && !(on0 && l2 == l0) && !(on1 && l2 == l1)) a[l2] += 1;
    }
    if (fresh || inside) {
      st.nc[slot] = (uint16_t)nc;
      st.cnt[slot] = (uint16_t)cn;
    }
    if (g < front1) {
      const int64_t j = g - lo;                          // < ST_RING
      emit_frame(nc, cn, a, K, cap2, count + (int64_t)r * ST_RING + j, speakers + ((int64_t)r * ST_RING + j) * 2);
    }
  }
  if (tid == 0) {
    st.hdr->K = K;
    st.hdr->frontier = max(front1, lo);
    st.hdr->reach = max(reach0, reach1);
    emit_lo[r] = lo;
    emit_n[r] = (int32_t)max((int64_t)0, front1 - lo);
  }
}

// block = one stream: the frames from the frontier to the recording's end leave the ring; a frame no chunk has reached is empty
__global__ __launch_bounds__(ST_NT) void stream_flush_kernel(const int64_t* __restrict__ n_samples, const uint8_t* __restrict__ active, int cap2,
                                                             void* __restrict__ state, StreamLayout lay, int64_t* __restrict__ emit_lo,
                                                             int32_t* __restrict__ emit_n, uint8_t* __restrict__ count,
                                                             int32_t* __restrict__ speakers) {
  const int r = blockIdx.x, tid = threadIdx.x;
  if (!active[r]) return;
  const StreamView st = st_view(state, lay, r);
  const int K = st.hdr->K;
  const int64_t lo = st.hdr->frontier, reach = st.hdr->reach;
  const int64_t hi = min(max(dz_frames(n_samples[r]), lo), lo + ST_RING);
  __syncthreads();                                       // every thread has read the header before thread 0 renews it
  for (int64_t g = lo + tid; g < hi; g += ST_NT) {
    const int slot = (int)(g & (ST_RING - 1));
    const bool held = g < reach;
    const int64_t j = g - lo;
    emit_frame(held ? st.nc[slot] : 0, held ? st.cnt[slot] : 0, held ? st.act + (int64_t)slot * lay.stride : nullptr, K, cap2,
               count + (int64_t)r * ST_RING + j, speakers + ((int64_t)r * ST_RING + j) * 2);
  }
  if (tid == 0) {
    st.hdr->frontier = hi;
    emit_lo[r] = lo;
    emit_n[r] = (int32_t)(hi - lo);
  }
}

__global__ __launch_bounds__(ST_NT) void stream_reset_kernel(void* __restrict__ state, StreamLayout lay, int R, const uint8_t* __restrict__ which) {
  const int r = blockIdx.x * ST_NT + threadIdx.x;
  if (r >= R || (which && !which[r])) return;
  StreamHdr* h = st_view(state, lay, r).hdr;
  h->frontier = 0;
  h->reach = 0;
  h->K = 0;
  h->pad[0] = h->pad[1] = h->pad[2] = 0;
  for (int k = 0; k < ST_MAXK; ++k) h->n[k] = 0;
}

// block = one of the streams first .. first + gridDim.x - 1; the outputs are indexed from `first`
__global__ __launch_bounds__(ST_NT) void stream_centroids_kernel(const void* __restrict__ state, StreamLayout lay, int capacity, int d, int first,
                                                                 float* __restrict__ cent, int32_t* __restrict__ counts, int32_t* __restrict__ Kout,
                                                                 double* __restrict__ sums) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const StreamView st = st_view(const_cast<void*>(state), lay, first + b);
  const int K = st.hdr->K;
  for (int i = tid; i < capacity * d; i += ST_NT) {
    cent[(int64_t)b * capacity * d + i] = i / d < K ? (float)st.unit[i] : 0.f;
    if (sums) sums[(int64_t)b * capacity * d + i] = i / d < K ? st.sums[i] : 0.0;
  }
  for (int k = tid; k < capacity; k += ST_NT) counts[(int64_t)b * capacity + k] = k < K ? st.hdr->n[k] : 0;
  if (tid == 0) Kout[b] = K;
}

bool st_shape_ok(int R, int capacity, int d) {
  return R >= 1 && R <= (1 << 20) && capacity >= 1 && capacity <= ST_MAXK && d >= 64 && d <= DZ_MAX_D && d % 64 == 0;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

#define ST_SHAPE(name)                                                                                                              \
  SDK_REQUIRE(R >= 1 && R <= (1 << 20), name ": R=%d streams (1 .. 2^20)", R);                                                      \
  SDK_REQUIRE(capacity >= 1 && capacity <= ST_MAXK, name ": capacity=%d (1 .. %d speakers per stream)", capacity, ST_MAXK);         \
  SDK_REQUIRE(d >= 64 && d <= DZ_MAX_D && d % 64 == 0, name ": d=%d not supported (a multiple of 64, at most %d)", d, DZ_MAX_D)

#define ST_STATE(name)                                                                                                              \
  SDK_REQUIRE(state && aligned(state, 256), name ": state=%p must be a 256-byte aligned device pointer", (const void*)state);       \
  SDK_REQUIRE(state_bytes >= sdk_stream_state_bytes(R, capacity, d), name ": state block of %lld bytes, %lld needed",               \
              (long long)state_bytes, (long long)sdk_stream_state_bytes(R, capacity, d))

extern "C" int64_t sdk_stream_state_bytes(int R, int capacity, int d) {
  if (!st_shape_ok(R, capacity, d)) {
    sdk_set_error("sdk_stream_state_bytes: R=%d capacity=%d d=%d (R 1 .. 2^20, capacity 1 .. %d, d a multiple of 64 up to %d)", R, capacity, d, ST_MAXK,
                  DZ_MAX_D);
    return 0;
  }
  return (int64_t)R * st_layout(capacity, d).per;
}

extern "C" int sdk_stream_reset(sdk_ctx* ctx, void* state, int64_t state_bytes, int R, int capacity, int d, const uint8_t* which, void* stream) {
  SDK_REQUIRE(ctx, "sdk_stream_reset: null context");
  ST_SHAPE("sdk_stream_reset");
  ST_STATE("sdk_stream_reset");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)R * sizeof(StreamHdr));
  hipLaunchKernelGGL(stream_reset_kernel, dim3((unsigned)((R + ST_NT - 1) / ST_NT)), dim3(ST_NT), 0, (hipStream_t)stream, state, st_layout(capacity, d), R,
                     which);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_stream_step(sdk_ctx* ctx, const float* E, const int32_t* info, const uint8_t* cls, const int64_t* starts, const uint8_t* active,
                               const int64_t* n_end, int R, int F, int d, int capacity, int hop, int latency, double delta_new, int max_speakers, void* state,
                               int64_t state_bytes, int32_t* labels, float* score, int32_t* K, int64_t* emit_lo, int32_t* emit_n, uint8_t* count,
                               int32_t* speakers, void* stream) {
  SDK_REQUIRE(ctx, "sdk_stream_step: null context");
  ST_SHAPE("sdk_stream_step");
  SDK_REQUIRE(F >= 1 && F <= ST_RING, "sdk_stream_step: F=%d frames per chunk (1 .. %d, the ring)", F, ST_RING);
  SDK_REQUIRE(hop >= DZ_HOP, "sdk_stream_step: hop=%d samples (at least %d, one frame)", hop, DZ_HOP);
  SDK_REQUIRE(latency >= hop, "sdk_stream_step: latency=%d samples is below the step, hop=%d", latency, hop);
  SDK_REQUIRE((latency - hop) / DZ_HOP + hop / DZ_HOP + 2 <= ST_RING,
              "sdk_stream_step: latency=%d samples with hop=%d keeps %d frames between the frontier and the newest chunk; the ring holds %d", latency, hop,
              (latency - hop) / DZ_HOP + hop / DZ_HOP + 2, ST_RING);
  SDK_REQUIRE(delta_new >= 0.0 && delta_new <= 2.0, "sdk_stream_step: delta_new=%g (a cosine distance, 0 .. 2)", delta_new);
  SDK_REQUIRE(max_speakers >= 0, "sdk_stream_step: max_speakers=%d (0, 1 or 2; larger values do not bind)", max_speakers);
  SDK_REQUIRE(E && info && cls && starts && active && labels && score && K && emit_lo && emit_n && count && speakers,
              "sdk_stream_step: null argument (E=%p info=%p cls=%p starts=%p active=%p labels=%p score=%p K=%p emit_lo=%p emit_n=%p count=%p speakers=%p)",
              (const void*)E, (const void*)info, (const void*)cls, (const void*)starts, (const void*)active, (void*)labels, (void*)score, (void*)K,
              (void*)emit_lo, (void*)emit_n, (void*)count, (void*)speakers);
  SDK_REQUIRE(aligned(E, 4) && aligned(info, 4) && aligned(labels, 4) && aligned(score, 4) && aligned(K, 4) && aligned(emit_n, 4) && aligned(speakers, 4),
              "sdk_stream_step: misaligned argument (E=%p info=%p labels=%p score=%p K=%p emit_n=%p speakers=%p: 4 bytes)", (const void*)E,
              (const void*)info, (void*)labels, (void*)score, (void*)K, (void*)emit_n, (void*)speakers);
  SDK_REQUIRE(aligned(starts, 8) && aligned(emit_lo, 8) && aligned(n_end, 8), "sdk_stream_step: misaligned argument (starts=%p emit_lo=%p n_end=%p: 8 bytes)",
              (const void*)starts, (void*)emit_lo, (const void*)n_end);
  ST_STATE("sdk_stream_step");
  const StreamLayout lay = st_layout(capacity, d);
  ProfScope ps(ctx, stream, SDK_K_COPY, 6.0 * R * capacity * d, (double)R * (12.0 * d + 8.0 * capacity * d + F * (5.0 + 2.0 * lay.stride)));
  hipLaunchKernelGGL(stream_step_kernel, dim3(R), dim3(ST_NT), 0, (hipStream_t)stream, E, info, cls, starts, active, n_end, F, d, capacity,
                     (latency - hop) / DZ_HOP, delta_new, min(2, max_speakers), state, lay, labels, score, K, emit_lo, emit_n, count, speakers);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_stream_flush(sdk_ctx* ctx, const int64_t* n_samples, const uint8_t* active, int R, int capacity, int d, int max_speakers,
                                void* state, int64_t state_bytes, int64_t* emit_lo, int32_t* emit_n, uint8_t* count, int32_t* speakers,
                                void* stream) {
  SDK_REQUIRE(ctx, "sdk_stream_flush: null context");
  ST_SHAPE("sdk_stream_flush");
  SDK_REQUIRE(max_speakers >= 0, "sdk_stream_flush: max_speakers=%d (0, 1 or 2; larger values do not bind)", max_speakers);
  SDK_REQUIRE(n_samples && active && emit_lo && emit_n && count && speakers,
              "sdk_stream_flush: null argument (n_samples=%p active=%p emit_lo=%p emit_n=%p count=%p speakers=%p)", (const void*)n_samples,
              (const void*)active, (void*)emit_lo, (void*)emit_n, (void*)count, (void*)speakers);
  SDK_REQUIRE(aligned(n_samples, 8) && aligned(emit_lo, 8) && aligned(emit_n, 4) && aligned(speakers, 4),
              "sdk_stream_flush: misaligned argument (n_samples=%p emit_lo=%p: 8 bytes; emit_n=%p speakers=%p: 4 bytes)", (const void*)n_samples,
              (void*)emit_lo, (void*)emit_n, (void*)speakers);
  ST_STATE("sdk_stream_flush");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)R * ST_RING * 9.0);
  hipLaunchKernelGGL(stream_flush_kernel, dim3(R), dim3(ST_NT), 0, (hipStream_t)stream, n_samples, active, min(2, max_speakers), state,
                     st_layout(capacity, d), emit_lo, emit_n, count, speakers);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_stream_centroids(sdk_ctx* ctx, const void* state, int64_t state_bytes, int R, int capacity, int d, int first, int count,
                                    float* cent, int32_t* counts, int32_t* K, double* sums, void* stream) {
  SDK_REQUIRE(ctx, "sdk_stream_centroids: null context");
  ST_SHAPE("sdk_stream_centroids");
  SDK_REQUIRE(first >= 0 && count >= 1 && first <= R - count, "sdk_stream_centroids: streams first=%d .. first + count=%d - 1 of R=%d", first, count, R);
  SDK_REQUIRE(cent && counts && K && aligned(cent, 4) && aligned(counts, 4) && aligned(K, 4) && aligned(sums, 8),
              "sdk_stream_centroids: null or misaligned argument (cent=%p counts=%p K=%p: 4 bytes; sums=%p: 8 bytes, or NULL)", (void*)cent,
              (void*)counts, (void*)K, (void*)sums);
  ST_STATE("sdk_stream_centroids");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)count * capacity * (12.0 * d + 4.0));
  hipLaunchKernelGGL(stream_centroids_kernel, dim3(count), dim3(ST_NT), 0, (hipStream_t)stream, state, st_layout(capacity, d), capacity, d, first, cent,
                     counts, K, sums);
  SDK_LAUNCH_CHECK();
  return 0;
}
