// Masked attentive statistics pooling: the two HBM sweeps of sdk_ecapa_forward_masked (forward_ecapa.hip), S weighted poolings per chunk on ONE
// trunk output h [B*T, C].  THE RULE (include/sdk_hip.h states it in full): for chunk b and slot s < S, w = w[b][s][0..T) >= 0 (any
// non-negative weights, not only 0 / 1), v1 = sum_t w_t:
//   context    mu_c = sum_t w_t h_tc / v1,  sd_c = sqrt(max(sum_t w_t (h_tc - mu_c)^2 / v1, 1e-12))          (asp_stats_masked)
//   attention  m_c = max over {t : w_t > 0} of l_tc,  e_tc = w_t exp(l_tc - m_c),  alpha_tc = e_tc / sum_t e_tc;  a frame with w_t = 0
//              enters neither the maximum nor any sum - its logit may be NaN or +inf                              (asp_pool_masked)
//   pooled     wmu_c = sum_t alpha_tc h_tc,  wsd_c = sqrt(max(sum_t alpha_tc (h_tc - wmu_c)^2, 1e-12))
// A row depends on its own weights only.  Rows with valid[b][s] == 0 are written as zeros and their weights are never used for a
// division; a row with valid != 0 and no weight (v1 <= 0; for the pool: no frame with w > 0) is written as zeros too (ZEROED, not
// refused: the weights live on the device).  With w == 1 this is sdk_asp_stats / sdk_asp_pool.
// Both kernels: channels on lanes, 16-byte loads, fp32 arithmetic, the frame group of a thread is its WAVE (so a frame's weights are
// wave-uniform: scalar loads), every thread sums its frames in order and the four groups meet in LDS as (0 + 1) + (2 + 3): bit-identical
// run to run, no atomics.  All row arithmetic on B T C is in 64 bits.
#include "common.hpp"

namespace {

constexpr int MK_NT = 256;          // 4 waves = 4 frame groups
constexpr int MK_SC = 512;          // channels per workgroup of the statistics sweep (8 per lane)
constexpr int MK_PC = 256;          // channels per workgroup of the pooling sweep (4 per lane)
constexpr int MK_SMAX = 8;

// ------------------------------------------------------------------------------------------
// Weighted mean / std over frames for all S slots of a chunk in one read of h: grid (B, ceil(C / 512)).  Sweep 1: a[s] = sum_t w_st h_t and
// v1[s] = sum_t w_st, every loaded value used S times; sweep 2 (the block's slab again: T x 1 KiB, from cache): sum_t w_st (h_t - mu_s)^2.
// Two passes, so nothing cancels: the variance is a sum of non-negative terms about the rounded mean.
template <int S, bool F16>
__global__ __launch_bounds__(MK_NT) void asp_stats_masked_kernel(const bf16_t* __restrict__ h, int64_t ldh, int T, int C,
                                                                const float* __restrict__ w, const int32_t* __restrict__ valid,
                                                                float* __restrict__ out, int32_t* __restrict__ ok_out) {
  __shared__ __attribute__((aligned(16))) float red[4][MK_SC];
  __shared__ __attribute__((aligned(16))) float mus[S][MK_SC];
  __shared__ float v1p[4][MK_SMAX];
  const int tid = threadIdx.x, c8 = tid & 63;
  const int grp = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int cbase = blockIdx.y * MK_SC + c8 * 8;
  // lanes past the last channel re-read channels 0..7 (C >= 8) and write nothing: the sweeps stay branch-free
  const bf16_t* hp = h + (int64_t)b * T * ldh + (cbase < C ? cbase : 0);
  const float* wb = w + (int64_t)b * S * T;

  // four independent 16-byte loads in flight per lane; frames grp, grp + 4, ... in order
  auto sweep = [&](auto&& body) {
    int t = grp;
    for (; t + 12 < T; t += 16) {
      u32x4 r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = *reinterpret_cast<const u32x4*>(hp + (int64_t)(t + 4 * u) * ldh);
#pragma unroll
      for (int u = 0; u < 4; ++u) body(r[u], t + 4 * u);
    }
    for (; t < T; t += 4) body(*reinterpret_cast<const u32x4*>(hp + (int64_t)t * ldh), t);
  };
  // the four groups' partial sums of slot s -> tot[c] for the block's 512 channels, in the order (0 + 1) + (2 + 3)
  auto store_part = [&](const float* p) {
    *reinterpret_cast<f32x4*>(&red[grp][c8 * 8]) = f32x4{p[0], p[1], p[2], p[3]};
    *reinterpret_cast<f32x4*>(&red[grp][c8 * 8 + 4]) = f32x4{p[4], p[5], p[6], p[7]};
  };

  float a[S][8], v[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    v[s] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[s][e] = 0.f;
  }
  sweep([&](const u32x4& raw, int t) {
    float f[8];
    unpack8t<F16>(raw, f);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float ws = wb[(int64_t)s * T + t];
      v[s] += ws;
#pragma unroll
      for (int e = 0; e < 8; ++e) a[s][e] = fmaf(ws, f[e], a[s][e]);
    }
  });
  if (c8 == 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) v1p[grp][s] = v[s];
  }
  float v1[S];
  bool ok[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    store_part(a[s]);
    __syncthreads();
    v1[s] = (v1p[0][s] + v1p[1][s]) + (v1p[2][s] + v1p[3][s]);
    ok[s] = valid[b * S + s] != 0 && v1[s] > 0.f;
    if (ok_out && blockIdx.y == 0 && tid == 0) ok_out[b * S + s] = ok[s] ? 1 : 0;
    for (int c = tid; c < MK_SC; c += MK_NT) {
      const float tot = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
      mus[s][c] = ok[s] ? tot / v1[s] : 0.f;
    }
    __syncthreads();
  }

  float m[S][8], q[S][8];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      m[s][e] = mus[s][c8 * 8 + e];
      q[s][e] = 0.f;
    }
  sweep([&](const u32x4& raw, int t) {
    float f[8];
    unpack8t<F16>(raw, f);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float ws = wb[(int64_t)s * T + t];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = f[e] - m[s][e];
        q[s][e] = fmaf(ws * d, d, q[s][e]);
      }
    }
  });
#pragma unroll
  for (int s = 0; s < S; ++s) {
    store_part(q[s]);
    __syncthreads();
    float* row = out + ((int64_t)b * S + s) * 2 * C;
    for (int c = tid; c < MK_SC; c += MK_NT) {
      const int cg = blockIdx.y * MK_SC + c;
      if (cg < C) {
        const float tot = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        row[cg] = mus[s][c];
        row[C + cg] = ok[s] ? sqrtf(var_floor(tot / v1[s])) : 0.f;
      }
    }
    __syncthreads();
  }
}

// 4 stored 2-byte elements (8 bytes) -> 4 floats
template <bool F16>
__device__ __forceinline__ void unpack4t(const u32x2& v, float* f) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t x = v[i];
    if constexpr (F16) {
      const f16x2_t t = __builtin_bit_cast(f16x2_t, x);
      f[2 * i] = (float)t[0];
      f[2 * i + 1] = (float)t[1];
    } else {
      f[2 * i] = __uint_as_float(x << 16);
      f[2 * i + 1] = __uint_as_float(x & 0xffff0000u);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Softmax over the frames with w > 0 and the weighted moments, for ONE slot s of every chunk (its logits [B*T, C] fp32): grid (B, ceil(C / 256)),
// lane = 4 channels (one 16-byte logit load, one 8-byte h load per frame), wave = frame group.  Three sweeps as asp_pool_kernel: maximum;
// sum e and sum e h; sum e (h - mu)^2.  Frames are taken 4 per group at a time and a run of 16 frames without weight is skipped whole (a
// speaker's activity is a few contiguous runs): neither its logits nor its h are read.
template <bool F16>
__global__ __launch_bounds__(MK_NT) void asp_pool_masked_kernel(const float* __restrict__ logits, int64_t ldl, const bf16_t* __restrict__ h,
                                                               int64_t ldh, int T, int C, int S, int s, const float* __restrict__ w,
                                                               const int32_t* __restrict__ valid, float* __restrict__ pooled) {
  __shared__ __attribute__((aligned(16))) float red[4][MK_PC];
  __shared__ __attribute__((aligned(16))) float red2[4][MK_PC];
  const int tid = threadIdx.x, lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int c0 = blockIdx.y * MK_PC + lane * 4;
  const bool live = c0 < C;                                         // C % 4 == 0: a live lane owns 4 channels
  float* row = pooled + ((int64_t)b * S + s) * 2 * C;
  if (valid[b * S + s] == 0) {                                      // block-uniform: the weights of an invalid row are never read
    if (g == 0 && live) {
      *reinterpret_cast<f32x4*>(row + c0) = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(row + C + c0) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const int cl = live ? c0 : 0;                                     // lanes past the last channel re-read channels 0..3 and write nothing
  const float* wr = w + ((int64_t)b * S + s) * T;
  const float* lp = logits + (int64_t)b * T * ldl + cl;
  const bf16_t* hp = h + (int64_t)b * T * ldh + cl;

  auto put4 = [&](float (*dst)[MK_PC], const float* p) { *reinterpret_cast<f32x4*>(&dst[g][lane * 4]) = f32x4{p[0], p[1], p[2], p[3]}; };
  auto sum4 = [&](float (*src)[MK_PC], float* p) {
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = (src[0][lane * 4 + e] + src[1][lane * 4 + e]) + (src[2][lane * 4 + e] + src[3][lane * 4 + e]);
  };
  // frames g, g + 4, ... in order, four at a time; body(weight > 0, logits, h) only for frames with weight
  auto sweep = [&](auto&& body) {
    int t = g;
    for (; t + 12 < T; t += 16) {
      float wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) wv[u] = wr[t + 4 * u];
      if (!(wv[0] > 0.f || wv[1] > 0.f || wv[2] > 0.f || wv[3] > 0.f)) continue;
      f32x4 lv[4];
      u32x2 hv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        lv[u] = *reinterpret_cast<const f32x4*>(lp + (int64_t)(t + 4 * u) * ldl);
        hv[u] = *reinterpret_cast<const u32x2*>(hp + (int64_t)(t + 4 * u) * ldh);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (wv[u] > 0.f) body(wv[u], lv[u], hv[u]);
    }
    for (; t < T; t += 4) {
      const float wv = wr[t];
      if (wv > 0.f) body(wv, *reinterpret_cast<const f32x4*>(lp + (int64_t)t * ldl), *reinterpret_cast<const u32x2*>(hp + (int64_t)t * ldh));
    }
  };

  float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  {                                                                 // the maximum needs no h: its own loop
    int t = g;
    for (; t + 12 < T; t += 16) {
      float wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) wv[u] = wr[t + 4 * u];
      if (!(wv[0] > 0.f || wv[1] > 0.f || wv[2] > 0.f || wv[3] > 0.f)) continue;
      f32x4 lv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) lv[u] = *reinterpret_cast<const f32x4*>(lp + (int64_t)(t + 4 * u) * ldl);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (wv[u] > 0.f) {
#pragma unroll
          for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], lv[u][e]);
        }
    }
    for (; t < T; t += 4)
      if (wr[t] > 0.f) {
        const f32x4 lv = *reinterpret_cast<const f32x4*>(lp + (int64_t)t * ldl);
#pragma unroll
        for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], lv[e]);
      }
  }
  put4(red, mx);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e)
    mx[e] = fmaxf(fmaxf(red[0][lane * 4 + e], red[1][lane * 4 + e]), fmaxf(red[2][lane * 4 + e], red[3][lane * 4 + e]));
  __syncthreads();

  float l[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
  sweep([&](float wv, const f32x4& lv, const u32x2& hv) {
    float f[4];
    unpack4t<F16>(hv, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ex = wv * __expf(lv[e] - mx[e]);
      l[e] += ex;
      s1[e] += ex * f[e];
    }
  });
  put4(red, l);
  put4(red2, s1);
  __syncthreads();
  sum4(red, l);
  sum4(red2, s1);
  __syncthreads();
  float mu[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) mu[e] = s1[e] / l[e];

  float s2[4] = {0.f, 0.f, 0.f, 0.f};
  sweep([&](float wv, const f32x4& lv, const u32x2& hv) {
    float f[4];
    unpack4t<F16>(hv, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ex = wv * __expf(lv[e] - mx[e]);
      const float d = f[e] - mu[e];
      s2[e] += ex * d * d;
    }
  });
  put4(red, s2);
  __syncthreads();
  if (g == 0 && live) {
    sum4(red, s2);
    f32x4 om, os;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool none = l[e] == 0.f;                                // no frame with weight: zeros (the frame of the maximum alone adds w > 0)
      om[e] = none ? 0.f : mu[e];
      os[e] = none ? 0.f : sqrtf(var_floor(s2[e] / l[e]));
    }
    *reinterpret_cast<f32x4*>(row + c0) = om;
    *reinterpret_cast<f32x4*>(row + C + c0) = os;
  }
}

template <bool F16>
int stats_masked_launch(int S, dim3 grid, hipStream_t st, const bf16_t* h, int64_t ldh, int T, int C, const float* w, const int32_t* valid, float* out,
                        int32_t* ok_out) {
  switch (S) {
#define MK_CASE(n) case n: hipLaunchKernelGGL((asp_stats_masked_kernel<n, F16>), grid, dim3(MK_NT), 0, st, h, ldh, T, C, w, valid, out, ok_out); return 0;
    MK_CASE(1) MK_CASE(2) MK_CASE(3) MK_CASE(4) MK_CASE(5) MK_CASE(6) MK_CASE(7) MK_CASE(8)
#undef MK_CASE
  }
  return 2;
}

}  // namespace

int asp_stats_masked_impl(sdk_ctx* ctx, const uint16_t* h, int64_t ldh, int B, int T, int C, int S, const float* w, const int32_t* valid, float* out_ctx,
                          void* stream, bool f16, int32_t* ok_out) {
  SDK_REQUIRE(ctx, "sdk_asp_stats_masked: ctx is null");
  SDK_REQUIRE(h && w && valid && out_ctx, "sdk_asp_stats_masked: null pointer (h=%p w=%p valid=%p out_ctx=%p)", (const void*)h, (const void*)w,
              (const void*)valid, (void*)out_ctx);
  SDK_REQUIRE(S >= 1 && S <= MK_SMAX, "sdk_asp_stats_masked: S=%d weight rows per chunk (served: 1 .. %d)", S, MK_SMAX);
  SDK_REQUIRE(B > 0 && T > 0 && C > 0 && C % 8 == 0 && ldh % 8 == 0 && ldh >= C && ((uintptr_t)h % 16) == 0,
              "sdk_asp_stats_masked: bad shape (B=%d T=%d C=%d ldh=%lld: C and ldh multiples of 8, ldh >= C, h 16-byte aligned)", B, T, C, (long long)ldh);
  SDK_REQUIRE((int64_t)B * S < (1ll << 31) && ((uintptr_t)out_ctx % 4) == 0 && ((uintptr_t)w % 4) == 0, "sdk_asp_stats_masked: B S = %lld rows, or a misaligned fp32 pointer",
              (long long)B * S);
  ProfScope ps(ctx, stream, SDK_K_ASP_STATS, (2.0 + 3.0) * S * B * T * C, 2.0 * B * T * C);
  const dim3 grid(B, ceil_div(C, MK_SC));
  const int rc = f16 ? stats_masked_launch<true>(S, grid, (hipStream_t)stream, (const bf16_t*)h, ldh, T, C, w, valid, out_ctx, ok_out)
                     : stats_masked_launch<false>(S, grid, (hipStream_t)stream, (const bf16_t*)h, ldh, T, C, w, valid, out_ctx, ok_out);
  SDK_REQUIRE(rc == 0, "sdk_asp_stats_masked: S=%d not built", S);
  SDK_LAUNCH_CHECK();
  return 0;
}

int asp_pool_masked_impl(sdk_ctx* ctx, const float* logits, int64_t ldl, const uint16_t* h, int64_t ldh, int B, int T, int C, int S, int s, const float* w,
                         const int32_t* valid, float* pooled, void* stream, bool f16) {
  SDK_REQUIRE(ctx, "sdk_asp_pool_masked: ctx is null");
  SDK_REQUIRE(logits && h && w && valid && pooled, "sdk_asp_pool_masked: null pointer (logits=%p h=%p w=%p valid=%p pooled=%p)", (const void*)logits,
              (const void*)h, (const void*)w, (const void*)valid, (void*)pooled);
  SDK_REQUIRE(S >= 1 && S <= MK_SMAX && s >= 0 && s < S, "sdk_asp_pool_masked: S=%d weight rows per chunk (served: 1 .. %d), slot s=%d", S, MK_SMAX, s);
  SDK_REQUIRE(B > 0 && T > 0 && C > 0 && C % 64 == 0, "sdk_asp_pool_masked: C=%d must be a multiple of 64 (B=%d T=%d)", C, B, T);
  SDK_REQUIRE(ldl % 4 == 0 && ldl >= C && ldh % 8 == 0 && ldh >= C && ((uintptr_t)logits % 16) == 0 && ((uintptr_t)h % 16) == 0 && ((uintptr_t)pooled % 16) == 0,
              "sdk_asp_pool_masked: ldl=%lld (a multiple of 4, >= C), ldh=%lld (a multiple of 8, >= C); logits, h and pooled 16-byte aligned", (long long)ldl,
              (long long)ldh);
  SDK_REQUIRE((int64_t)B * S < (1ll << 31), "sdk_asp_pool_masked: B S = %lld rows", (long long)B * S);
  ProfScope ps(ctx, stream, SDK_K_ASP_POOL, 8.0 * B * T * C, 6.0 * B * T * C);
  hipLaunchKernelGGL(f16 ? asp_pool_masked_kernel<true> : asp_pool_masked_kernel<false>, dim3(B, ceil_div(C, MK_PC)), dim3(MK_NT), 0, (hipStream_t)stream, logits,
                     ldl, (const bf16_t*)h, ldh, T, C, S, s, w, valid, pooled);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_asp_stats_masked_fmt(sdk_ctx* ctx, const uint16_t* h, int64_t ldh, int B, int T, int C, int S, const float* w, const int32_t* valid,
                                        float* out_ctx, int precision, void* stream) {
  SDK_REQUIRE(precision == 0 || precision == 2, "sdk_asp_stats_masked_fmt: precision=%d (0: bf16 elements, 2: fp16 elements; the precise mode's planes are not served)",
              precision);
  return asp_stats_masked_impl(ctx, h, ldh, B, T, C, S, w, valid, out_ctx, stream, precision == 2, nullptr);
}

extern "C" int sdk_asp_pool_masked_fmt(sdk_ctx* ctx, const float* logits, int64_t ldl, const uint16_t* h, int64_t ldh, int B, int T, int C, int S, int s,
                                       const float* w, const int32_t* valid, float* pooled, int precision, void* stream) {
  SDK_REQUIRE(precision == 0 || precision == 2, "sdk_asp_pool_masked_fmt: precision=%d (0: bf16 elements, 2: fp16 elements; the precise mode's planes are not served)",
              precision);
  return asp_pool_masked_impl(ctx, logits, ldl, h, ldh, B, T, C, S, s, w, valid, pooled, stream, precision == 2);
}
