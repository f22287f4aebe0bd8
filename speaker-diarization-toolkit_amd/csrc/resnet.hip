// ResNet34 embedding family (resnet.py, sdk_resnet_forward): the 2-D convolutions and the temporal statistics pooling.
//
// resnet_conv_kernel - a 3x3 conv (zero padding 1, stride 1 or 2) as an implicit GEMM on the 16x16x32 MFMA.  GEMM rows are output positions
// (b, fo, to) of channel-last activations [B][F][T][C], K = 9 Cin tap-major (k = (3 dy + dx) Cin + c), W [Cout][K] K-contiguous.  A workgroup
// owns 64 output positions of one segment - an R x W block of (fo, to), R W = 64, picked per layer to waste the fewest rows at the map's edges -
// and every output channel (the tile's N = Cout: 32 / 64 / 128 / 256).  Per CK-channel chunk of the input it stages the halo'd patch
// ((R-1) s + 3) x ((W-1) s + 3) x CK into LDS once, zero-filled outside the image, and builds all nine taps' operands from it: each input
// element crosses L2 -> CU once per tile, not nine times, and there is no im2col buffer.  A Cin = 32 tap is exactly one K-slice.
// Operand roles: A = W (rows = output channels), B = the patch (columns = positions), so each accumulator holds 4 consecutive channels of one
// position; the two channel blocks of a pair take the rows 8 (r >> 2) + 4 h + (r & 3), and a lane ends up with 8 consecutive channels of a
// position - stored as one 16-byte chunk, the identity residual read the same way.  Epilogue in fp32: + bias (the folded BN shift)
// [+ residual] [ReLU], rounded once to the 2-byte storage format.  A projection shortcut is extra K columns: its 1x1 strided input is read
// straight from global memory (each element is used by one position only) against W's last Csc columns, inside the same accumulators.
#include "common.hpp"

namespace {

constexpr int RN_NT = 256;     // 4 waves
constexpr int RN_POS = 64;     // output positions per workgroup

struct ConvGeo {
  int F, T, Fo, To, Cin, Cout;
  int R, W, nFb, nTb, PR, PC;  // tile rows / columns (R W = 64), tiles per segment along f / t, LDS patch rows / columns
  int Csc, Fsc, Tsc, ssc;
  int ldw;
};

template <int NTILE, int S, int CK, bool F16>
__global__ __launch_bounds__(RN_NT) void resnet_conv_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ Wt, const float* __restrict__ bias,
                                                            const bf16_t* __restrict__ sc, const bf16_t* __restrict__ res, bf16_t* __restrict__ y,
                                                            ConvGeo g, int relu) {
  constexpr int WN = NTILE >= 128 ? 4 : NTILE / 32;   // waves along the channels
  constexpr int WM = 4 / WN;                          // waves along the positions
  constexpr int CB = NTILE / 16 / WN;                 // 16-channel blocks per wave (even: pairs)
  constexpr int PB = 4 / WM;                          // 16-position blocks per wave
  constexpr int PS = CK + 8;                          // LDS elements per patch position (+16 bytes: the b128 operand reads spread over the banks)
  static_assert(CB % 2 == 0 && PB >= 1, "tile split");
  extern __shared__ __attribute__((aligned(16))) bf16_t patch[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wn = wid % WN, wm = wid / WN;
  const int l15 = lane & 15, lg = lane >> 4;
  int tile = blockIdx.x;
  const int tb = tile % g.nTb;
  tile /= g.nTb;
  const int fb = tile % g.nFb;
  const int b = tile / g.nFb;
  const int fo0 = fb * g.R, to0 = tb * g.W;
  const int fi0 = fo0 * S - 1, ti0 = to0 * S - 1;

  // B operand (patch): lane holds position l15 of each of its position blocks, channels 8 lg .. 8 lg + 7 of the K-slice
  int poff[PB];
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    const int pos = (wm * PB + p) * 16 + l15;
    const int r = pos / g.W, w = pos - r * g.W;
    poff[p] = ((r * S) * g.PC + w * S) * PS + 8 * lg;
  }
  // A operand (W): lane holds row l15 of each channel block = channel n0 + 32 (cb / 2) + 8 (l15 >> 2) + 4 (cb & 1) + (l15 & 3)
  const int n0 = wn * (NTILE / WN);
  const bf16_t* wrow[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
    wrow[cb] = Wt + (int64_t)(n0 + 32 * (cb >> 1) + 8 * (l15 >> 2) + 4 * (cb & 1) + (l15 & 3)) * g.ldw + 8 * lg;

  f32x4 acc[CB][PB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int p = 0; p < PB; ++p) acc[cb][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int npos = g.PR * g.PC;
  for (int cc = 0; cc < g.Cin; cc += CK) {
    if (cc) __syncthreads();                           // every wave is done with the previous chunk's patch
    for (int i = threadIdx.x; i < npos * (CK / 8); i += RN_NT) {
      const int q = i % (CK / 8), pp = i / (CK / 8);
      const int pr = pp / g.PC, pc = pp - pr * g.PC;
      const int fi = fi0 + pr, ti = ti0 + pc;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (fi >= 0 && fi < g.F && ti >= 0 && ti < g.T)
        v = *reinterpret_cast<const u32x4*>(x + (((int64_t)b * g.F + fi) * g.T + ti) * g.Cin + cc + 8 * q);
      *reinterpret_cast<u32x4*>(patch + pp * PS + 8 * q) = v;
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = ((tap / 3) * g.PC + (tap % 3)) * PS;
#pragma unroll
      for (int sub = 0; sub < CK / 32; ++sub) {
        const int k0 = tap * g.Cin + cc + 32 * sub;
        bf16x8 a[CB], bb[PB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) a[cb] = *reinterpret_cast<const bf16x8*>(wrow[cb] + k0);
#pragma unroll
        for (int p = 0; p < PB; ++p) bb[p] = *reinterpret_cast<const bf16x8*>(patch + poff[p] + toff + 32 * sub);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int p = 0; p < PB; ++p) acc[cb][p] = mfma_16x16x32<F16>(a[cb], bb[p], acc[cb][p]);
      }
    }
  }

  // output positions of this lane (clamped into the map for the loads; positions outside it are not stored)
  int fo[PB], to[PB];
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    const int pos = (wm * PB + p) * 16 + l15;
    const int r = pos / g.W;
    fo[p] = fo0 + r;
    to[p] = to0 + pos - r * g.W;
  }
  if (sc) {
    const bf16_t* sp[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p)
      sp[p] = sc + (((int64_t)b * g.Fsc + min(fo[p], g.Fo - 1) * g.ssc) * g.Tsc + min(to[p], g.To - 1) * g.ssc) * g.Csc + 8 * lg;
    const int kb = 9 * g.Cin;
    for (int kc = 0; kc < g.Csc; kc += 32) {
      bf16x8 a[CB], bb[PB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) a[cb] = *reinterpret_cast<const bf16x8*>(wrow[cb] + kb + kc);
#pragma unroll
      for (int p = 0; p < PB; ++p) bb[p] = *reinterpret_cast<const bf16x8*>(sp[p] + kc);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int p = 0; p < PB; ++p) acc[cb][p] = mfma_16x16x32<F16>(a[cb], bb[p], acc[cb][p]);
    }
  }
#pragma unroll
  for (int p = 0; p < PB; ++p) {
    if (fo[p] >= g.Fo || to[p] >= g.To) continue;
    const int64_t o = (((int64_t)b * g.Fo + fo[p]) * g.To + to[p]) * g.Cout;
#pragma unroll
    for (int q = 0; q < CB / 2; ++q) {
      const int ch = n0 + 32 * q + 8 * lg;
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[2 * q][p][i] + bias[ch + i];
        v[4 + i] = acc[2 * q + 1][p][i] + bias[ch + 4 + i];
      }
      if (res) {
        float rv[8];
        unpack8t<F16>(*reinterpret_cast<const u32x4*>(res + o + ch), rv);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += rv[i];
      }
      if (relu) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
      }
      *reinterpret_cast<u32x4*>(y + o + ch) = pack8t<F16>(v);
    }
  }
}

// The stem (Cin = 1, 3x3, stride 1, 32 output channels) on the vector ALUs: K = 9 would fill 9 / 32 of an MFMA K-slice, and the layer is
// bound by its 64-byte-per-position output stream anyway.  Thread = one output position (t fastest: the stores of a wave are contiguous).
template <bool F16>
__global__ __launch_bounds__(RN_NT) void resnet_stem_kernel(const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ Wt,
                                                            const float* __restrict__ bias, bf16_t* __restrict__ y, int B, int F, int T, int relu) {
  __shared__ float ws[32 * 9];
  __shared__ float bs[32];
  for (int i = threadIdx.x; i < 32 * 9; i += RN_NT) ws[i] = load1t<F16>(Wt + i);
  if (threadIdx.x < 32) bs[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * RN_NT + threadIdx.x;
  if (idx >= (int64_t)B * F * T) return;
  const int t = (int)(idx % T);
  const int64_t bf = idx / T;
  const int f = (int)(bf % F), b = (int)(bf / F);
  float in[9];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int fi = f + dy - 1, ti = t + dx - 1;
      in[3 * dy + dx] = (fi >= 0 && fi < F && ti >= 0 && ti < T) ? load1t<F16>(x + ((int64_t)b * T + ti) * ldx + fi) : 0.f;
    }
  bf16_t* out = y + idx * 32;
#pragma unroll
  for (int c8 = 0; c8 < 4; ++c8) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 8 * c8 + e;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) s = fmaf(ws[9 * c + k], in[k], s);
      s += bs[c];
      v[e] = relu ? fmaxf(s, 0.f) : s;
    }
    *reinterpret_cast<u32x4*>(out + 8 * c8) = pack8t<F16>(v);
  }
}

// Temporal statistics pooling of the last map [B][F][T][C]: feature c F + f (the public flatten order) -> out[b] = mean (2-pass, fp32) |
// sqrt(unbiased var + 1e-7).  Workgroup = (segment, f); lanes over channels (coalesced 2-byte reads), the frames in order.
template <bool F16>
__global__ __launch_bounds__(RN_NT) void resnet_tstp_kernel(const bf16_t* __restrict__ x, int F, int T, int C, float* __restrict__ out) {
  const int b = blockIdx.x / F, f = blockIdx.x % F;
  const float invT = 1.0f / (float)T, invT1 = 1.0f / (float)(T - 1);
  float* o = out + (int64_t)b * 2 * C * F;
  for (int c = threadIdx.x; c < C; c += RN_NT) {
    const bf16_t* p = x + ((int64_t)b * F + f) * T * C + c;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += load1t<F16>(p + (int64_t)t * C);
    const float mean = s * invT;
    float q = 0.f;
    for (int t = 0; t < T; ++t) {
      const float d = load1t<F16>(p + (int64_t)t * C) - mean;
      q = fmaf(d, d, q);
    }
    o[c * F + f] = mean;
    o[C * F + c * F + f] = sqrtf(q * invT1 + 1e-7f);
  }
}

// The same statistics with a weight per (speaker, frame): S rows per segment from ONE sweep of the last map (diarize.py: the conv trunk runs
// once per chunk, the speakers of a chunk differ only here).  w [B][S][T] fp32 >= 0, valid [B][S]; out row b S + s.  With v1 = sum w,
// v2 = sum w^2: mean = sum w x / v1, var = sum w (x - mean)^2 / (v1 - v2 / v1), std = sqrt(var + 1e-7) - for 0 / 1 weights the unbiased
// statistic over the selected frames.  Two passes, fp32, frames in order; a row's result depends on its own weights only.  Rows with
// valid == 0 are zeros.  Workgroup = (segment, f), lanes over channels as above; the weights sit in LDS, the speakers go in groups of MP_SG so
// that a group's pass reads each map element once (S = 3: one group).
constexpr int MP_SG = 4;
template <bool F16>
__global__ __launch_bounds__(RN_NT) void resnet_masked_tstp_kernel(const bf16_t* __restrict__ x, int F, int T, int C, int S, const float* __restrict__ w,
                                                                   const int32_t* __restrict__ valid, float* __restrict__ out) {
  extern __shared__ float wl[];                        // [S][T]
  const int b = blockIdx.x / F, f = blockIdx.x % F;
  for (int i = threadIdx.x; i < S * T; i += RN_NT) wl[i] = w[(int64_t)b * S * T + i];
  __syncthreads();
  for (int s0 = 0; s0 < S; s0 += MP_SG) {
    const int ns = min(MP_SG, S - s0);
    float v1[MP_SG], v2[MP_SG];
    bool ok[MP_SG];
#pragma unroll
    for (int i = 0; i < MP_SG; ++i) {
      v1[i] = 0.f; v2[i] = 0.f;
      ok[i] = i < ns && valid[b * S + s0 + i] != 0;
      const float* ws = wl + (s0 + min(i, ns - 1)) * T;
      for (int t = 0; t < T; ++t) { v1[i] += ws[t]; v2[i] = fmaf(ws[t], ws[t], v2[i]); }
    }
    for (int c = threadIdx.x; c < C; c += RN_NT) {
      const bf16_t* p = x + ((int64_t)b * F + f) * T * C + c;
      float sum[MP_SG], q[MP_SG], mean[MP_SG];
#pragma unroll
      for (int i = 0; i < MP_SG; ++i) { sum[i] = 0.f; q[i] = 0.f; }
      for (int t = 0; t < T; ++t) {
        const float v = load1t<F16>(p + (int64_t)t * C);
#pragma unroll
        for (int i = 0; i < MP_SG; ++i) sum[i] = fmaf(wl[(s0 + min(i, ns - 1)) * T + t], v, sum[i]);
      }
#pragma unroll
      for (int i = 0; i < MP_SG; ++i) mean[i] = sum[i] / v1[i];
      for (int t = 0; t < T; ++t) {
        const float v = load1t<F16>(p + (int64_t)t * C);
#pragma unroll
        for (int i = 0; i < MP_SG; ++i) {
          const float d = v - mean[i];
          q[i] = fmaf(wl[(s0 + min(i, ns - 1)) * T + t] * d, d, q[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < MP_SG; ++i) {
        if (i >= ns) continue;
        float* o = out + ((int64_t)b * S + s0 + i) * 2 * C * F;
        o[c * F + f] = ok[i] ? mean[i] : 0.f;
        o[C * F + c * F + f] = ok[i] ? sqrtf(q[i] / (v1[i] - v2[i] / v1[i]) + 1e-7f) : 0.f;
      }
    }
  }
}

// rows with valid == 0 -> zeros (after seg_1, whose bias would otherwise be their value)
__global__ __launch_bounds__(RN_NT) void resnet_zero_invalid_kernel(float* __restrict__ emb, int n, int dim, const int32_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * RN_NT + threadIdx.x;
  if (i < (int64_t)n * dim && valid[i / dim] == 0) emb[i] = 0.f;
}

// tile shape: fewest computed positions (edges of the map), then the smallest patch
void pick_tile(int Fo, int To, int s, int* R, int* W) {
  int64_t best = -1, bestp = 0;
  for (int w = 8; w <= 64; w *= 2) {
    const int r = RN_POS / w;
    const int64_t cost = (int64_t)ceil_div(Fo, r) * ceil_div(To, w) * RN_POS;
    const int64_t pt = (int64_t)((r - 1) * s + 3) * ((w - 1) * s + 3);
    if (best < 0 || cost < best || (cost == best && pt < bestp)) { best = cost; bestp = pt; *R = r; *W = w; }
  }
}

template <int NTILE, int S, int CK, bool F16>
void launch_conv(const sdk_resnet_conv_args* a, const ConvGeo& g, int nblk, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL((resnet_conv_kernel<NTILE, S, CK, F16>), dim3(nblk), dim3(RN_NT), lds, st, (const bf16_t*)a->x, (const bf16_t*)a->W, a->bias,
                     (const bf16_t*)a->sc, (const bf16_t*)a->res, (bf16_t*)a->y, g, (int)(a->flags & SDK_GEMM_RELU));
}

template <int NTILE, bool F16>
int dispatch_conv(const sdk_resnet_conv_args* a, const ConvGeo& g, int nblk, size_t lds, hipStream_t st) {
  const bool ck32 = a->Cin == 32;
  if (a->stride == 1) {
    if (ck32) launch_conv<NTILE, 1, 32, F16>(a, g, nblk, lds, st);
    else launch_conv<NTILE, 1, 64, F16>(a, g, nblk, lds, st);
  } else {
    if (ck32) launch_conv<NTILE, 2, 32, F16>(a, g, nblk, lds, st);
    else launch_conv<NTILE, 2, 64, F16>(a, g, nblk, lds, st);
  }
  return 0;
}

bool resnet_width_ok(int c) { return c == 32 || c == 64 || c == 128 || c == 256; }

}  // namespace

extern "C" int sdk_resnet_conv2d(sdk_ctx* ctx, const sdk_resnet_conv_args* a, void* stream) {
  SDK_REQUIRE(ctx && a && a->x && a->W && a->bias && a->y, "sdk_resnet_conv2d: null argument");
  SDK_REQUIRE(a->B > 0 && a->F > 0 && a->T > 0, "sdk_resnet_conv2d: empty image (B=%d F=%d T=%d)", a->B, a->F, a->T);
  SDK_REQUIRE(a->stride == 1 || a->stride == 2, "sdk_resnet_conv2d: stride=%d (1 or 2)", a->stride);
  SDK_REQUIRE((a->flags & ~(SDK_GEMM_RELU | SDK_GEMM_F16)) == 0, "sdk_resnet_conv2d: flags=0x%x (SDK_GEMM_RELU | SDK_GEMM_F16 only)", a->flags);
  const bool f16 = a->flags & SDK_GEMM_F16;
  const int Fo = (a->F - 1) / a->stride + 1, To = (a->T - 1) / a->stride + 1;
  const hipStream_t st = (hipStream_t)stream;
  if (a->Cin == 1) {
    SDK_REQUIRE(a->Cout == 32 && a->stride == 1 && !a->sc && !a->res && a->Csc == 0 && a->ldx >= a->F && ((uintptr_t)a->y % 16) == 0,
                "sdk_resnet_conv2d: the stem (Cin = 1) has Cout = 32, stride 1, no shortcut / residual, ldx >= F (Cout=%d stride=%d ldx=%lld F=%d)",
                a->Cout, a->stride, (long long)a->ldx, a->F);
    // the kernel indexes in int64; only the grid size is int32: ceil_div((int)n, RN_NT) must not overflow
    const int64_t n = (int64_t)a->B * a->F * a->T;
    SDK_REQUIRE(n < (1ll << 31) - RN_NT, "sdk_resnet_conv2d: image too large (stem: B*F*T=%lld output positions, at most 2^31 - %d)", (long long)n,
                RN_NT + 1);
    ProfScope ps(ctx, stream, SDK_K_RESNET_STEM, 2.0 * a->B * a->F * a->T * 32 * 9, 2.0 * a->B * a->F * a->T * (1 + 32));
    hipLaunchKernelGGL(f16 ? resnet_stem_kernel<true> : resnet_stem_kernel<false>, dim3((unsigned)ceil_div((int)n, RN_NT)), dim3(RN_NT), 0, st,
                       (const bf16_t*)a->x, a->ldx, (const bf16_t*)a->W, a->bias, (bf16_t*)a->y, a->B, a->F, a->T, (int)(a->flags & SDK_GEMM_RELU));
    SDK_LAUNCH_CHECK();
    return 0;
  }
  SDK_REQUIRE(resnet_width_ok(a->Cin) && resnet_width_ok(a->Cout), "sdk_resnet_conv2d: Cin=%d Cout=%d (each 32, 64, 128 or 256; Cin = 1: the stem)",
              a->Cin, a->Cout);
  SDK_REQUIRE(((uintptr_t)a->x % 16) == 0 && ((uintptr_t)a->W % 16) == 0 && ((uintptr_t)a->y % 16) == 0 && ((uintptr_t)a->res % 16) == 0 &&
              ((uintptr_t)a->sc % 16) == 0, "sdk_resnet_conv2d: x, W, sc, res and y must be 16-byte aligned (x=%p W=%p sc=%p res=%p y=%p)",
              (const void*)a->x, (const void*)a->W, (const void*)a->sc, (const void*)a->res, (const void*)a->y);
  SDK_REQUIRE(!(a->sc && a->res), "sdk_resnet_conv2d: a projection shortcut and an identity residual exclude each other");
  if (a->sc) {
    SDK_REQUIRE(resnet_width_ok(a->Csc) && (a->stride_sc == 1 || a->stride_sc == 2) && (a->Fsc - 1) / a->stride_sc + 1 == Fo &&
                (a->Tsc - 1) / a->stride_sc + 1 == To && a->Fsc > 0 && a->Tsc > 0,
                "sdk_resnet_conv2d: shortcut input [%d][%d][%d] at stride %d does not map onto the %d x %d output", a->Fsc, a->Tsc, a->Csc,
                a->stride_sc, Fo, To);
  } else {
    SDK_REQUIRE(a->Csc == 0, "sdk_resnet_conv2d: Csc=%d without a shortcut input", a->Csc);
  }
  SDK_REQUIRE((int64_t)a->B * a->F * a->T * a->Cin < (1ll << 40), "sdk_resnet_conv2d: image too large");
  ConvGeo g;
  g.F = a->F; g.T = a->T; g.Fo = Fo; g.To = To; g.Cin = a->Cin; g.Cout = a->Cout;
  pick_tile(Fo, To, a->stride, &g.R, &g.W);
  g.nFb = ceil_div(Fo, g.R); g.nTb = ceil_div(To, g.W);
  g.PR = (g.R - 1) * a->stride + 3; g.PC = (g.W - 1) * a->stride + 3;
  g.Csc = a->sc ? a->Csc : 0; g.Fsc = a->Fsc; g.Tsc = a->Tsc; g.ssc = a->stride_sc;
  g.ldw = 9 * a->Cin + g.Csc;
  const int ck = a->Cin == 32 ? 32 : 64;
  const size_t lds = (size_t)g.PR * g.PC * (ck + 8) * 2;
  const int64_t nblk = (int64_t)a->B * g.nFb * g.nTb;
  SDK_REQUIRE(nblk < (1ll << 31), "sdk_resnet_conv2d: too many tiles");
  const double M = (double)a->B * Fo * To;
  ProfScope ps(ctx, stream, SDK_K_RESNET_CONV, 2.0 * M * a->Cout * g.ldw,
               2.0 * ((double)a->B * a->F * a->T * a->Cin + M * a->Cout * (a->res ? 2 : 1) + M * g.Csc + (double)a->Cout * g.ldw));
  const int nb = (int)nblk;
  switch (a->Cout) {
    case 32: f16 ? dispatch_conv<32, true>(a, g, nb, lds, st) : dispatch_conv<32, false>(a, g, nb, lds, st); break;
    case 64: f16 ? dispatch_conv<64, true>(a, g, nb, lds, st) : dispatch_conv<64, false>(a, g, nb, lds, st); break;
    case 128: f16 ? dispatch_conv<128, true>(a, g, nb, lds, st) : dispatch_conv<128, false>(a, g, nb, lds, st); break;
    default: f16 ? dispatch_conv<256, true>(a, g, nb, lds, st) : dispatch_conv<256, false>(a, g, nb, lds, st); break;
  }
  SDK_LAUNCH_CHECK();
  return 0;
}

int resnet_tstp_impl(sdk_ctx* ctx, const uint16_t* x, int B, int F, int T, int C, float* out, void* stream, bool f16) {
  SDK_REQUIRE(ctx && x && out, "resnet pooling: null argument");
  SDK_REQUIRE(B > 0 && F > 0 && T >= 2 && C > 0, "resnet pooling: the last map has %d frames; the unbiased variance needs >= 2 (segments of >= 9 frames)", T);
  ProfScope ps(ctx, stream, SDK_K_RESNET_POOL, 4.0 * B * F * T * C, 2.0 * B * F * T * C + 8.0 * B * F * C);
  hipLaunchKernelGGL(f16 ? resnet_tstp_kernel<true> : resnet_tstp_kernel<false>, dim3(B * F), dim3(RN_NT), 0, (hipStream_t)stream, (const bf16_t*)x, F, T, C, out);
  SDK_LAUNCH_CHECK();
  return 0;
}

int resnet_masked_tstp_impl(sdk_ctx* ctx, const uint16_t* x, int B, int F, int T, int C, int S, const float* w, const int32_t* valid, float* out,
                            void* stream, bool f16) {
  SDK_REQUIRE(ctx && x && w && valid && out, "resnet masked pooling: null argument");
  SDK_REQUIRE(B > 0 && F > 0 && T >= 2 && C > 0, "resnet masked pooling: the last map has %d frames; the unbiased variance needs >= 2 (B=%d F=%d C=%d)", T, B, F, C);
  SDK_REQUIRE(S >= 1 && (int64_t)S * T * 4 <= 48 * 1024, "resnet masked pooling: S=%d weight rows of %d frames (S >= 1, S T <= 12288: they are staged in LDS)", S, T);
  SDK_REQUIRE((int64_t)B * F < (1ll << 31) && (int64_t)B * S < (1ll << 31), "resnet masked pooling: batch too large (B=%d F=%d S=%d)", B, F, S);
  ProfScope ps(ctx, stream, SDK_K_RESNET_POOL, 4.0 * B * F * T * C * S, 2.0 * B * F * T * C + 8.0 * B * S * F * C + 4.0 * B * S * T);
  hipLaunchKernelGGL(f16 ? resnet_masked_tstp_kernel<true> : resnet_masked_tstp_kernel<false>, dim3(B * F), dim3(RN_NT), (size_t)S * T * 4, (hipStream_t)stream,
                     (const bf16_t*)x, F, T, C, S, w, valid, out);
  SDK_LAUNCH_CHECK();
  return 0;
}

int resnet_zero_invalid_impl(sdk_ctx* ctx, float* emb, int n, int dim, const int32_t* valid, void* stream) {
  SDK_REQUIRE(ctx && emb && valid && n > 0 && dim > 0 && (int64_t)n * dim < (1ll << 31) - RN_NT, "resnet masked rows: bad argument (n=%d dim=%d)", n, dim);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 4.0 * n * dim);
  hipLaunchKernelGGL(resnet_zero_invalid_kernel, dim3(ceil_div(n * dim, RN_NT)), dim3(RN_NT), 0, (hipStream_t)stream, emb, n, dim, valid);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_resnet_masked_pool(sdk_ctx* ctx, const uint16_t* x, int B, int F, int T, int C, int S, const float* w, const int32_t* valid,
                                      float* out, int fmt, void* stream) {
  SDK_REQUIRE(fmt == 0 || fmt == 2, "sdk_resnet_masked_pool: fmt=%d (0: bf16, 2: fp16; the precise mode is not built for the ResNet34 family)", fmt);
  return resnet_masked_tstp_impl(ctx, x, B, F, T, C, S, w, valid, out, stream, fmt == 2);
}

extern "C" int sdk_resnet_pool(sdk_ctx* ctx, const uint16_t* x, int B, int F, int T, int C, float* out, int fmt, void* stream) {
  SDK_REQUIRE(fmt == 0 || fmt == 2, "sdk_resnet_pool: fmt=%d (0: bf16, 2: fp16; the precise mode is not built for the ResNet34 family)", fmt);
  SDK_REQUIRE((int64_t)B * F < (1ll << 31), "sdk_resnet_pool: batch too large (B=%d F=%d)", B, F);
  return resnet_tstp_impl(ctx, x, B, F, T, C, out, stream, fmt == 2);
}
