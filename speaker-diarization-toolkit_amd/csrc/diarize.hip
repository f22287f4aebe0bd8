// Speaker diarization (diarize.py): the integer stages that join the segmentation model, the ResNet34 embedding and the clustering.
//
//   powerset_decode_kernel     logp [C][F][7] -> cls [C][F]: the argmax class, ties to the lower class.  Everything later reads cls.
//   diarize_masks_kernel       cls [B][F] -> the pooling weights of sdk_resnet_forward_masked, w [B][3][T4], and info [B][3][4] per
//                              (chunk, local speaker): (active frames, clean frames, used_clean, valid).
//   diarize_reconstruct_kernel cls, chunk starts, labels [C][3] -> count [G], speakers [G][2] (and act [G][K]) on the global frame grid of
//                              segmentation.aggregate_counts.
//
// Every kernel is a gather: one owner per output element, integer arithmetic (the weights are 0 / 1), no atomics, so the results are
// bit-identical run to run.
#include "common.hpp"

namespace {

constexpr int DZ_NT = 256;
constexpr int DZ_HOP = 270;          // samples between segmentation frames
constexpr int DZ_MIN_CLEAN = 4;      // columns of the last map a speaker needs alone before the overlapped ones are dropped (diarize.MIN_CLEAN_COLUMNS)

// the speakers of powerset class c = {}, {0}, {1}, {2}, {0,1}, {0,2}, {1,2} as a 3-bit mask (0 for anything else)
__device__ __forceinline__ int cls_mask(int c) { return (unsigned)c < 7u ? (0x6534210 >> (4 * c)) & 7 : 0; }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

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
    act[s] = wave_sum_i(act[s]);
    cln[s] = wave_sum_i(cln[s]);
    colf[s] = wave_sum_i(colf[s]);
    colc[s] = wave_sum_i(colc[s]);
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

// q_c = floor((135 - start_c) / 270): global frame g reads frame g + q_c of chunk c
__device__ __forceinline__ int64_t chunk_q(int64_t start) {
  const int64_t a = 135 - start;
  return a >= 0 ? a / DZ_HOP : -((-a + DZ_HOP - 1) / DZ_HOP);
}

// thread = one global frame.  The starts ascend, so q_c never grows with c: the chunks with g + q_c >= 0 are a prefix, those with
// g + q_c < F a suffix, and the chunks that see the frame are the range between two binary searches.
__global__ __launch_bounds__(DZ_NT) void diarize_reconstruct_kernel(const uint8_t* __restrict__ cls, const int32_t* __restrict__ starts,
                                                                    const int32_t* __restrict__ labels, int C, int F, int K, int G, int max_speakers,
                                                                    uint8_t* __restrict__ count, int32_t* __restrict__ speakers,
                                                                    int32_t* __restrict__ act) {
  const int g = blockIdx.x * DZ_NT + threadIdx.x;
  if (g >= G) return;
  int lo = 0, hi = C;                                  // first chunk with g + q_c < F
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g + chunk_q(starts[mid]) < F) hi = mid; else lo = mid + 1;
  }
  const int c0 = lo;
  lo = 0; hi = C;                                      // first chunk with g + q_c < 0
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
    if (act) act[(int64_t)g * K + k] = a;
    if (a > a1) { a2 = a1; k2 = k1; a1 = a; k1 = k; }
    else if (a > a2) { a2 = a; k2 = k; }
  }
  int n = nc ? (2 * cnt + nc) / (2 * nc) : 0;           // the mean count, rounded half up
  n = min(n, min(2, max_speakers));
  count[g] = (uint8_t)n;
  speakers[2 * (int64_t)g] = n >= 1 ? k1 : -1;
  speakers[2 * (int64_t)g + 1] = n >= 2 ? k2 : -1;
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

extern "C" int64_t sdk_diarize_frames(int64_t n_samples) {
  const int64_t g = (n_samples - 495 + DZ_HOP - 1) / DZ_HOP;
  return n_samples < 495 || g < 0 ? 0 : g;
}

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
