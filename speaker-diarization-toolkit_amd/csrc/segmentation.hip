// PyanNet speaker segmentation (segmentation.py, sdk_segmentation_forward): SincNet front end, 4-layer BiLSTM, head.
//
// seg_wavstats_kernel - per chunk: sum x and sum x^2 of the int16 samples in int64 (exact), mean / biased variance in float64 -> the
//   waveform InstanceNorm as one affine map x -> a x + b, applied after the sinc conv: conv(a x + b) = a conv(x) + b sum(w).
// seg_convpool_kernel - a 1-D conv whose window for output position t is the contiguous slice [t es, t es + K) of the chunk's flat row
//   (sinc: es = 10 samples, Cin = 1; convs 2 / 3: es = Cin-padded row, taps x channels tap-major), as an MFMA GEMM with A = W (rows =
//   channels) and B = windows (columns = positions); fused MaxPool1d(3, 3).  A workgroup owns 64 pooled positions = 192 conv positions of one
//   chunk, staged once in LDS; a wave owns 16 pooled positions, and its three row blocks are the three conv positions of every pool, so the
//   pool is a max over three accumulators of one lane.  Every activation operand is staged as hi + lo 2-byte planes (two MFMAs per product):
//   the int16 samples split exactly, the fp32 maps of convs 2 / 3 split on the way in.  The sinc layer applies the affine waveform norm and
//   |.| before the pool.  Output: fp32 pooled maps [B][Lp][16 NB].
// seg_inorm_kernel - InstanceNorm1d (affine) + LeakyReLU(0.01) of one chunk's pooled map: two-pass float64 statistics over the positions in
//   a fixed order, fp32 output (zero-padded channels up to ldo).
// seg_proj_kernel - the LSTM input projection of both directions, G [M][1024] fp32 = x W_ih^T + (b_ih + b_hh), x split into planes.
// seg_lstm_kernel - the recurrence: persistent, one workgroup per (16 chunks, direction), all F steps in one launch.  W_hh (512 x 128) lives in
//   VGPRs as MFMA fragments: wave w owns the four gates of hidden units 32 w .. 32 w + 31, so each lane holds i, f, g, o of the same
//   (unit, chunk) and the cell update stays in the lane.  c stays in fp32 registers; h goes to the layer output in fp32 and, as hi + lo
//   planes, through a double-buffered LDS tile (one barrier per step) into the next step's MFMAs.
// seg_head_kernel - Linear(256, 128) + LeakyReLU and Linear(128, 128) + LeakyReLU on MFMAs over planes, Linear(128, 7) and log_softmax in fp32.
// Every reduction runs in a fixed order: results are deterministic run to run.
#include "common.hpp"

namespace {

constexpr int SG_NT = 256;
constexpr int SG_POOL_TILE = 64;      // pooled positions per conv workgroup
constexpr int SG_SINC_TAPS = 251;
constexpr int SG_SINC_K = 256;        // taps padded to the MFMA K step
constexpr int SG_SINC_STRIDE = 10;
constexpr int SG_HID = 128;
constexpr int SG_GATES = 4 * SG_HID;
constexpr int SG_LSTM_TILE = 16;      // chunks per recurrence workgroup
constexpr int SG_HPAD = SG_HID + 8;   // LDS row of h (+16 bytes: spreads the b128 operand reads over the banks)


__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.01f * v; }
__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }

template <bool F16>
__device__ __forceinline__ uint16_t to_bits(float v) {
  if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)sat_f16(v));
  else return __builtin_bit_cast(uint16_t, (bf16_t)v);
}
template <bool F16>
__device__ __forceinline__ float from_bits(uint16_t v) {
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, v);
  else return __uint_as_float((uint32_t)v << 16);
}

// an fp32 operand as two 2-byte planes: hi = round(v), lo = round(v - hi) (v - hi is exact in fp32)
template <bool F16>
__device__ __forceinline__ void split2(float v, uint16_t* hi, uint16_t* lo) {
  *hi = to_bits<F16>(v);
  *lo = to_bits<F16>(v - from_bits<F16>(*hi));
}
template <bool F16>
__device__ __forceinline__ void split8(const float* v, bf16x8* hi, bf16x8* lo) {
  uint16_t h[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) split2<F16>(v[e], &h[e], &l[e]);
  u32x4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = (uint32_t)h[2 * i] | ((uint32_t)h[2 * i + 1] << 16);
    b[i] = (uint32_t)l[2 * i] | ((uint32_t)l[2 * i + 1] << 16);
  }
  *hi = __builtin_bit_cast(bf16x8, a);
  *lo = __builtin_bit_cast(bf16x8, b);
}

// first sample of chunk b and the number of its samples that exist (the rest read as zero)
__device__ __forceinline__ void chunk_base(const int32_t* starts, int64_t n_samples, int ld, int S, int b, int64_t* base, int64_t* avail) {
  if (starts) {
    *base = starts[b];
    *avail = n_samples - *base;
  } else {
    *base = (int64_t)b * ld;
    *avail = S;
  }
}

__global__ __launch_bounds__(SG_NT) void seg_wavstats_kernel(const int16_t* __restrict__ x, int64_t n_samples, const int32_t* __restrict__ starts,
                                                             int ld, int S, const float* __restrict__ wn, float* __restrict__ ab) {
  __shared__ long long r1[SG_NT], r2[SG_NT];
  const int b = blockIdx.x;
  int64_t base, avail;
  chunk_base(starts, n_samples, ld, S, b, &base, &avail);
  const int lim = (int)(avail < S ? avail : S);
  long long s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < lim; i += SG_NT) {
    const long long v = base + i >= 0 ? x[base + i] : 0;
    s1 += v;
    s2 += v * v;
  }
  r1[threadIdx.x] = s1;
  r2[threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t1 = 0, t2 = 0;                  // integer sums: exact in any order
    for (int i = 0; i < SG_NT; ++i) { t1 += r1[i]; t2 += r2[i]; }
    const double mean = (double)t1 / S;
    const double var = fmax(((double)t2 - (double)t1 * mean) / S, 0.0);
    const double a = (double)wn[0] / sqrt(var + 1e-5);
    ab[2 * b] = (float)a;
    ab[2 * b + 1] = (float)((double)wn[1] - mean * a);
  }
}

struct ConvPoolGeo {
  // sinc source
  const int16_t* samples; int64_t n_samples; const int32_t* starts; int ld; int S;
  // conv source: x [B][Lin][ldc] fp32
  const float* x; int Lin; int ldc;
  const bf16_t* W; int K;          // W [16 NB][K] 2-byte, K % 32 == 0 (zero-padded)
  const float* bias;               // [16 NB] (conv) or NULL
  const float* wsum;               // [16 NB] sum of the rounded sinc taps (sinc)
  const float* ab;                 // [B][2] waveform norm (sinc)
  float* P; int Lp;                // pooled output [B][Lp][16 NB] fp32
  int es;                          // elements per conv position step
  int span;                        // staged elements per tile: 191 es + K (multiple of 8)
};

template <bool F16, bool SINC, int NB>
__global__ __launch_bounds__(SG_NT) void seg_convpool_kernel(ConvPoolGeo g) {
  extern __shared__ __attribute__((aligned(16))) uint16_t stage[];   // hi plane [span] then lo plane [span]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int ntile = (g.Lp + SG_POOL_TILE - 1) / SG_POOL_TILE;
  const int b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
  const int64_t pos0 = (int64_t)tile * 3 * SG_POOL_TILE;     // first conv position of the tile

  if constexpr (SINC) {
    int64_t base, avail;
    chunk_base(g.starts, g.n_samples, g.ld, g.S, b, &base, &avail);
    const int64_t lim = avail < g.S ? avail : g.S;
    const int64_t e0 = pos0 * SG_SINC_STRIDE;
    for (int i = threadIdx.x; i < g.span; i += SG_NT) {
      const int64_t e = e0 + i;
      const float v = (e < lim && base + e >= 0) ? (float)g.samples[base + e] : 0.f;
      const uint16_t hi = to_bits<F16>(v);
      stage[i] = hi;
      stage[g.span + i] = to_bits<F16>(v - from_bits<F16>(hi));   // exact: the remainder has <= 8 (bf16) / 5 (fp16) significant bits
    }
  } else {
    const int64_t rowlen = (int64_t)g.Lin * g.ldc;
    const int64_t e0 = pos0 * g.es;
    const float* src = g.x + (int64_t)b * rowlen;
    for (int i = 4 * threadIdx.x; i < g.span; i += 4 * SG_NT) {   // 4 fp32 -> 4 elements of each plane (rowlen and span are multiples of 4)
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (e0 + i < rowlen) v = *reinterpret_cast<const f32x4*>(src + e0 + i);
      uint16_t h[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) split2<F16>(v[e], &h[e], &l[e]);
      *reinterpret_cast<u32x2*>(stage + i) = u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
      *reinterpret_cast<u32x2*>(stage + g.span + i) = u32x2{(uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16)};
    }
  }
  __syncthreads();

  f32x4 acc[NB][3];
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int r = 0; r < 3; ++r) acc[n][r] = f32x4{0.f, 0.f, 0.f, 0.f};
  int boff[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) boff[r] = (3 * (16 * wid + l15) + r) * g.es + 8 * lg;
  const bf16_t* wrow = g.W + (int64_t)l15 * g.K + 8 * lg;

  for (int k0 = 0; k0 < g.K; k0 += 32) {
    bf16x8 a[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) a[n] = *reinterpret_cast<const bf16x8*>(wrow + (int64_t)16 * n * g.K + k0);
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
      bf16x8 bb[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        if constexpr (SINC) {
          const uint32_t* q = reinterpret_cast<const uint32_t*>(stage + plane * g.span + boff[r] + k0);   // 4-byte aligned (even offset)
          u32x4 v = {q[0], q[1], q[2], q[3]};
          bb[r] = __builtin_bit_cast(bf16x8, v);
        } else {
          bb[r] = *reinterpret_cast<const bf16x8*>(stage + plane * g.span + boff[r] + k0);   // 16-byte aligned: es, span % 8 == 0
        }
      }
#pragma unroll
      for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[n][r] = mfma_16x16x32<F16>(a[n], bb[r], acc[n][r]);
    }
  }

  const int p = tile * SG_POOL_TILE + 16 * wid + l15;
  if (p >= g.Lp) return;
  float sa = 0.f, sb = 0.f;
  if constexpr (SINC) {
    sa = g.ab[2 * b];
    sb = g.ab[2 * b + 1];
  }
  float* out = g.P + ((int64_t)b * g.Lp + p) * (16 * NB);
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int ch = 16 * n + 4 * lg;
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        if constexpr (SINC) v[r] = fabsf(fmaf(sa, acc[n][r][i], sb * g.wsum[ch + i]));
        else v[r] = acc[n][r][i] + g.bias[ch + i];
      }
      o[i] = fmaxf(fmaxf(v[0], v[1]), v[2]);
    }
    *reinterpret_cast<f32x4*>(out + ch) = o;
  }
}

// InstanceNorm1d(C, affine) + LeakyReLU of P [B][L][ldp] fp32 -> y [B][L][ldo] fp32 (channels C .. ldo - 1 zero).  Thread (part, c): the
// positions l = part, part + nparts, ... in order; the parts are summed in order.  The sums run in float64: an fp32 running sum over the
// ~1 800 positions of a thread (10-s chunks) loses more than the fp32 reference's own error.
__global__ __launch_bounds__(SG_NT) void seg_inorm_kernel(const float* __restrict__ P, int L, int ldp, int C, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ y, int ldo) {
  __shared__ double red[SG_NT];
  __shared__ float stat[2][128];
  const int b = blockIdx.x;
  const int nparts = SG_NT / C;
  const int c = threadIdx.x % C, part = threadIdx.x / C;
  const float* src = P + (int64_t)b * L * ldp;
  const bool act = part < nparts;
  double s = 0.0;
  if (act)
    for (int l = part; l < L; l += nparts) s += (double)src[(int64_t)l * ldp + c];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < C) {
    double t = 0.0;
    for (int q = 0; q < nparts; ++q) t += red[q * C + threadIdx.x];
    stat[0][threadIdx.x] = (float)(t / L);
  }
  __syncthreads();
  const float mean = stat[0][c];
  double q2 = 0.0;
  if (act)
    for (int l = part; l < L; l += nparts) {
      const double d = (double)src[(int64_t)l * ldp + c] - (double)mean;
      q2 = fma(d, d, q2);
    }
  __syncthreads();
  red[threadIdx.x] = q2;
  __syncthreads();
  if (threadIdx.x < C) {
    double t = 0.0;
    for (int q = 0; q < nparts; ++q) t += red[q * C + threadIdx.x];
    stat[1][threadIdx.x] = (float)(1.0 / sqrt(t / L + 1e-5));
  }
  __syncthreads();
  float* dst = y + (int64_t)b * L * ldo;
  const int64_t n = (int64_t)L * ldo;
  for (int64_t i = threadIdx.x; i < n; i += SG_NT) {
    const int l = (int)(i / ldo), cc = (int)(i - (int64_t)l * ldo);
    float v = 0.f;
    if (cc < C) v = leaky(fmaf(gamma[cc] * stat[1][cc], src[(int64_t)l * ldp + cc] - stat[0][cc], beta[cc]));
    dst[i] = v;
  }
}

// G [M][1024] fp32 = x [M][ldx] (fp32, first Kin columns, as hi + lo planes) . W [1024][Kp]^T + bias.  Tile 64 rows x 256 columns; wave = 64
// columns.
template <bool F16>
__global__ __launch_bounds__(SG_NT) void seg_proj_kernel(const float* __restrict__ x, int ldx, int Kin, int M, const bf16_t* __restrict__ W, int Kp,
                                                         const float* __restrict__ bias, float* __restrict__ G) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * 64;
  const int n0 = blockIdx.y * 256 + 64 * wid;
  f32x4 acc[4][4];
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Kp; k0 += 32) {
    bf16x8 a[4], bb[4], bl[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) a[n] = *reinterpret_cast<const bf16x8*>(W + (int64_t)(n0 + 16 * n + l15) * Kp + k0 + 8 * lg);
    const int kk = k0 + 8 * lg;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t row = m0 + 16 * m + l15;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (row < M && kk < Kin) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + row * ldx + kk), v1 = *reinterpret_cast<const f32x4*>(x + row * ldx + kk + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = kk + e < Kin ? v0[e] : 0.f;
          v[4 + e] = kk + 4 + e < Kin ? v1[e] : 0.f;
        }
      }
      split8<F16>(v, &bb[m], &bl[m]);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc[n][m] = mfma_16x16x32<F16>(a[n], bb[m], acc[n][m]);
        acc[n][m] = mfma_16x16x32<F16>(a[n], bl[m], acc[n][m]);
      }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int64_t row = m0 + 16 * m + l15;
    if (row >= M) continue;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = n0 + 16 * n + 4 * lg;
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = acc[n][m][i] + bias[col + i];
      *reinterpret_cast<f32x4*>(G + row * 1024 + col) = o;
    }
  }
}

// One BiLSTM layer's recurrence.  G [B][F][1024] fp32 (direction d at columns 512 d + gate row, rows i | f | g | o of 128), Whh [2][512][128]
// 2-byte, y [B][F][256] fp32 (direction d at columns 128 d).  h_{t-1} enters the MFMAs as hi + lo planes.  grid (ceil(B / 16), 2).
template <bool F16>
__global__ __launch_bounds__(SG_NT) void seg_lstm_kernel(const float* __restrict__ G, const bf16_t* __restrict__ Whh, float* __restrict__ y, int B, int F) {
  __shared__ __attribute__((aligned(16))) uint16_t hbuf[2][2][SG_LSTM_TILE][SG_HPAD];     // [buffer][hi | lo][chunk][unit]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int dir = blockIdx.y;
  const int b = blockIdx.x * SG_LSTM_TILE + l15;
  const bool valid = b < B;
  for (int i = threadIdx.x; i < 4 * SG_LSTM_TILE * SG_HPAD; i += SG_NT) (&hbuf[0][0][0][0])[i] = 0;

  // W_hh fragments: row block rb = 2 q + hh -> gate rows 128 q + 32 wid + 16 hh + (0..15); k-slices ks of the hidden units
  bf16x8 a[8][4];
  const bf16_t* wd = Whh + (int64_t)dir * SG_GATES * SG_HID;
#pragma unroll
  for (int rb = 0; rb < 8; ++rb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      a[rb][ks] = *reinterpret_cast<const bf16x8*>(wd + (int64_t)(128 * (rb >> 1) + 32 * wid + 16 * (rb & 1) + l15) * SG_HID + 32 * ks + 8 * lg);
  // this lane's gate rows in G / accumulators: 128 q + 32 wid + 16 hh + 4 lg + i
  const float* gb = G + (int64_t)(valid ? b : 0) * F * 1024 + dir * SG_GATES + 32 * wid + 4 * lg;
  float* yb = y + (int64_t)(valid ? b : 0) * F * 256 + dir * SG_HID + 32 * wid + 4 * lg;
  float c[2][4];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int i = 0; i < 4; ++i) c[hh][i] = 0.f;
  f32x4 gn[8];
  {
    const int t = dir ? F - 1 : 0;
#pragma unroll
    for (int rb = 0; rb < 8; ++rb)
      gn[rb] = valid ? *reinterpret_cast<const f32x4*>(gb + (int64_t)t * 1024 + 128 * (rb >> 1) + 16 * (rb & 1)) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  for (int s = 0; s < F; ++s) {
    const int t = dir ? F - 1 - s : s;
    const int cur = s & 1;
    f32x4 acc[8];
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) acc[rb] = gn[rb];
    if (s + 1 < F && valid) {                                  // next step's input projection, in flight under this step
      const int tn = dir ? t - 1 : t + 1;
#pragma unroll
      for (int rb = 0; rb < 8; ++rb) gn[rb] = *reinterpret_cast<const f32x4*>(gb + (int64_t)tn * 1024 + 128 * (rb >> 1) + 16 * (rb & 1));
    }
    bf16x8 hb[4], hl[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      hb[ks] = *reinterpret_cast<const bf16x8*>(&hbuf[cur][0][l15][32 * ks + 8 * lg]);
      hl[ks] = *reinterpret_cast<const bf16x8*>(&hbuf[cur][1][l15][32 * ks + 8 * lg]);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int rb = 0; rb < 8; ++rb) {
        acc[rb] = mfma_16x16x32<F16>(a[rb][ks], hb[ks], acc[rb]);
        acc[rb] = mfma_16x16x32<F16>(a[rb][ks], hl[ks], acc[rb]);
      }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      uint16_t hv[4], lv[4];
      f32x4 hf;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ig = sigm(acc[0 + hh][i]), fg = sigm(acc[2 + hh][i]), gg = tanhf(acc[4 + hh][i]), og = sigm(acc[6 + hh][i]);
        c[hh][i] = fg * c[hh][i] + ig * gg;
        hf[i] = og * tanhf(c[hh][i]);
        split2<F16>(hf[i], &hv[i], &lv[i]);
      }
      *reinterpret_cast<u32x2*>(&hbuf[cur ^ 1][0][l15][32 * wid + 16 * hh + 4 * lg]) =
          u32x2{(uint32_t)hv[0] | ((uint32_t)hv[1] << 16), (uint32_t)hv[2] | ((uint32_t)hv[3] << 16)};
      *reinterpret_cast<u32x2*>(&hbuf[cur ^ 1][1][l15][32 * wid + 16 * hh + 4 * lg]) =
          u32x2{(uint32_t)lv[0] | ((uint32_t)lv[1] << 16), (uint32_t)lv[2] | ((uint32_t)lv[3] << 16)};
      if (valid) *reinterpret_cast<f32x4*>(yb + (int64_t)t * 256 + 16 * hh) = hf;
    }
    lds_barrier();
  }
}

// Head of 64 frame rows per workgroup (16 per wave): x [M][256] fp32 -> logp [M][7] fp32.  x and the first hidden layer enter the MFMAs as
// hi + lo planes.
template <bool F16>
__global__ __launch_bounds__(SG_NT) void seg_head_kernel(const float* __restrict__ x, int M, const bf16_t* __restrict__ W1, const float* __restrict__ b1,
                                                         const bf16_t* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ Wc,
                                                         const float* __restrict__ bc, float* __restrict__ logp) {
  // the first hidden layer's planes [wave][hi | lo][row][unit], then (after a barrier) the second hidden layer [wave][row][unit] fp32
  __shared__ __attribute__((aligned(16))) float shm[4 * 2 * 16 * SG_HPAD / 2];
  uint16_t (*h1)[2][16][SG_HPAD] = reinterpret_cast<uint16_t (*)[2][16][SG_HPAD]>(shm);
  float (*h2)[16][SG_HID + 4] = reinterpret_cast<float (*)[16][SG_HID + 4]>(shm);
  static_assert(4 * 16 * (SG_HID + 4) <= 4 * 2 * 16 * SG_HPAD / 2, "head LDS");
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int64_t row = (int64_t)blockIdx.x * 64 + 16 * wid + l15;
  const bool valid = row < M;
  f32x4 acc[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < 256; k0 += 32) {
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + row * 256 + k0 + 8 * lg), v1 = *reinterpret_cast<const f32x4*>(x + row * 256 + k0 + 8 * lg + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = v0[e]; v[4 + e] = v1[e]; }
    }
    bf16x8 bb, bl;
    split8<F16>(v, &bb, &bl);
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const bf16x8 w = *reinterpret_cast<const bf16x8*>(W1 + (16 * n + l15) * 256 + k0 + 8 * lg);
      acc[n] = mfma_16x16x32<F16>(w, bb, acc[n]);
      acc[n] = mfma_16x16x32<F16>(w, bl, acc[n]);
    }
  }
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int u = 16 * n + 4 * lg;
    uint16_t hv[4], lv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split2<F16>(leaky(acc[n][i] + b1[u + i]), &hv[i], &lv[i]);
    *reinterpret_cast<u32x2*>(&h1[wid][0][l15][u]) = u32x2{(uint32_t)hv[0] | ((uint32_t)hv[1] << 16), (uint32_t)hv[2] | ((uint32_t)hv[3] << 16)};
    *reinterpret_cast<u32x2*>(&h1[wid][1][l15][u]) = u32x2{(uint32_t)lv[0] | ((uint32_t)lv[1] << 16), (uint32_t)lv[2] | ((uint32_t)lv[3] << 16)};
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 8; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k0 = 0; k0 < 128; k0 += 32) {
    const bf16x8 bb = *reinterpret_cast<const bf16x8*>(&h1[wid][0][l15][k0 + 8 * lg]);
    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&h1[wid][1][l15][k0 + 8 * lg]);
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const bf16x8 w = *reinterpret_cast<const bf16x8*>(W2 + (16 * n + l15) * 128 + k0 + 8 * lg);
      acc[n] = mfma_16x16x32<F16>(w, bb, acc[n]);
      acc[n] = mfma_16x16x32<F16>(w, bl, acc[n]);
    }
  }
  __syncthreads();                                             // every wave has read its planes: h2 overwrites them
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int u = 16 * n + 4 * lg;
#pragma unroll
    for (int i = 0; i < 4; ++i) h2[wid][l15][u + i] = leaky(acc[n][i] + b2[u + i]);
  }
  __syncthreads();
  // classifier: lane (part lg) sums its 32 units in order; the four parts are added in order by lane l15
  float z[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    float s = 0.f;
    for (int u = 32 * lg; u < 32 * lg + 32; ++u) s = fmaf(Wc[j * 128 + u], h2[wid][l15][u], s);
    const float p1 = __shfl(s, l15 + 16, 64), p2 = __shfl(s, l15 + 32, 64), p3 = __shfl(s, l15 + 48, 64);
    z[j] = ((s + p1) + p2) + p3 + bc[j];
  }
  if (lg != 0 || !valid) return;
  float mx = z[0];
#pragma unroll
  for (int j = 1; j < 7; ++j) mx = fmaxf(mx, z[j]);
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < 7; ++j) se += expf(z[j] - mx);
  const float lse = mx + logf(se);
  float* o = logp + row * 7;
#pragma unroll
  for (int j = 0; j < 7; ++j) o[j] = z[j] - lse;
}

// ------------------------------------------------------------------------------------------------ host side
int seg_frames(int S) {
  if (S < 991) return 0;
  const int l0 = (S - SG_SINC_TAPS) / SG_SINC_STRIDE + 1;
  return (((l0 / 3) - 4) / 3 - 4) / 3;
}
struct SegDims { int L0, L1, L2, F; };
SegDims seg_dims(int S) {
  SegDims d;
  d.L0 = (S - SG_SINC_TAPS) / SG_SINC_STRIDE + 1;
  d.L1 = d.L0 / 3;
  d.L2 = (d.L1 - 4) / 3;
  d.F = (d.L2 - 4) / 3;
  return d;
}

int check_sdesc(const sdk_segmentation_desc* d) {
  SDK_REQUIRE(d, "segmentation desc is null");
  SDK_REQUIRE(d->precision != 1, "segmentation desc: precision 1 (the precise mode) is not built for the segmentation model; use 0 (bf16) or 2 (fp16)");
  SDK_REQUIRE(d->precision == 0 || d->precision == 2, "segmentation desc: precision=%d (0: bf16 operands, 2: one fp16 plane)", d->precision);
  for (int i = 0; i < SDK_SEG_SLOTS; ++i)
    SDK_REQUIRE(d->off[i] >= 0 && d->off[i] % 256 == 0, "segmentation desc: slot %d missing or misaligned (off=%lld)", i, (long long)d->off[i]);
  return 0;
}

// the three work regions of the forward: R1 fp32 pooled maps and the gate pre-activations, R2 normalised 2-byte maps, R3 the LSTM output
struct SegWs { float *ab, *R1, *R2, *R3; };
size_t seg_carve(WsCarver c, int B, int S, SegWs* w) {
  const SegDims g = seg_dims(S);
  const size_t b = (size_t)B;
  size_t r1 = b * g.L1 * 80;
  r1 = r1 > b * g.L2 * 64 ? r1 : b * g.L2 * 64;
  const size_t r2 = r1;
  r1 = r1 > b * g.F * 1024 ? r1 : b * g.F * 1024;
  w->ab = c.take<float>(b * 2);
  w->R1 = c.take<float>(r1);
  w->R2 = c.take<float>(r2 + 16);
  w->R3 = c.take<float>(b * g.F * 256);
  return c.bytes();
}

template <bool F16, bool SINC, int NB>
int launch_convpool(sdk_ctx* ctx, const ConvPoolGeo& g, int B, hipStream_t st) {
  const size_t lds = (size_t)g.span * 2 * 2;                 // hi and lo planes
  const int ntile = ceil_div(g.Lp, SG_POOL_TILE);
  SDK_REQUIRE((int64_t)B * ntile < (1ll << 31), "segmentation: too many conv tiles (B=%d)", B);
  hipLaunchKernelGGL((seg_convpool_kernel<F16, SINC, NB>), dim3(B * ntile), dim3(SG_NT), lds, st, g);
  SDK_LAUNCH_CHECK();
  return 0;
}

template <bool F16>
int inorm(const float* P, int B, int L, int ldp, int C, const float* gb, float* y, int ldo, hipStream_t st) {
  hipLaunchKernelGGL(seg_inorm_kernel, dim3(B), dim3(SG_NT), 0, st, P, L, ldp, C, gb, gb + C, y, ldo);
  SDK_LAUNCH_CHECK();
  return 0;
}

// samples -> [B F][64] 2-byte frames (channels 60..63 zero), through R1 / R2 of the workspace
template <bool F16>
int frontend(sdk_ctx* ctx, const char* wb, const sdk_segmentation_desc* d, const int16_t* samples, int64_t n_samples, const int32_t* starts, int ld,
             int B, int S, char* ws, float* out, hipStream_t st) {
  const SegDims g = seg_dims(S);
  SegWs w;
  seg_carve({ws, 0}, B, S, &w);
  float *const ab = w.ab, *const R1 = w.R1, *const R2 = w.R2;
  auto F32 = [&](int s) { return (const float*)(wb + d->off[s]); };
  auto U16 = [&](int s) { return (const bf16_t*)(wb + d->off[s]); };
  hipLaunchKernelGGL(seg_wavstats_kernel, dim3(B), dim3(SG_NT), 0, st, samples, n_samples, starts, ld, S, F32(SDK_SEG_WAVNORM), ab);
  SDK_LAUNCH_CHECK();
  ConvPoolGeo c{};
  c = ConvPoolGeo{};
  c.samples = samples; c.n_samples = n_samples; c.starts = starts; c.ld = ld; c.S = S;
  c.W = U16(SDK_SEG_SINC); c.K = SG_SINC_K; c.wsum = F32(SDK_SEG_SINC_SUM); c.ab = ab;
  c.P = R1; c.Lp = g.L1; c.es = SG_SINC_STRIDE; c.span = (3 * SG_POOL_TILE - 1) * SG_SINC_STRIDE + SG_SINC_K;
  if (int rc = launch_convpool<F16, true, 5>(ctx, c, B, st)) return rc;
  if (int rc = inorm<F16>(R1, B, g.L1, 80, 80, F32(SDK_SEG_NORM0), R2, 80, st)) return rc;
  c = ConvPoolGeo{};                                  // Conv1d(80, 60, 5): K = 400 padded to 416
  c.x = R2; c.Lin = g.L1; c.ldc = 80; c.W = U16(SDK_SEG_CONV1_W); c.K = 416; c.bias = F32(SDK_SEG_CONV1_B);
  c.P = R1; c.Lp = g.L2; c.es = 80; c.span = (3 * SG_POOL_TILE - 1) * 80 + 416;
  if (int rc = launch_convpool<F16, false, 4>(ctx, c, B, st)) return rc;
  if (int rc = inorm<F16>(R1, B, g.L2, 64, 60, F32(SDK_SEG_NORM1), R2, 64, st)) return rc;
  c = ConvPoolGeo{};                                  // Conv1d(60, 60, 5) on 64-channel rows: K = 320
  c.x = R2; c.Lin = g.L2; c.ldc = 64; c.W = U16(SDK_SEG_CONV2_W); c.K = 320; c.bias = F32(SDK_SEG_CONV2_B);
  c.P = R1; c.Lp = g.F; c.es = 64; c.span = (3 * SG_POOL_TILE - 1) * 64 + 320;
  if (int rc = launch_convpool<F16, false, 4>(ctx, c, B, st)) return rc;
  return inorm<F16>(R1, B, g.F, 64, 60, F32(SDK_SEG_NORM2), out, 64, st);
}

template <bool F16>
int bilstm(const char* wb, const sdk_segmentation_desc* d, int layer, const float* x, int ldx, int B, int F, float* G, float* y, hipStream_t st) {
  const int Kin = layer ? 256 : 60, Kp = layer ? 256 : 64;
  const int64_t M = (int64_t)B * F;
  hipLaunchKernelGGL(seg_proj_kernel<F16>, dim3((unsigned)((M + 63) / 64), 4), dim3(SG_NT), 0, st, x, ldx, Kin, (int)M,
                     (const bf16_t*)(wb + d->off[SDK_SEG_LSTM + 3 * layer]), Kp, (const float*)(wb + d->off[SDK_SEG_LSTM + 3 * layer + 1]), G);
  SDK_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_lstm_kernel<F16>, dim3(ceil_div(B, SG_LSTM_TILE), 2), dim3(SG_NT), 0, st, (const float*)G,
                     (const bf16_t*)(wb + d->off[SDK_SEG_LSTM + 3 * layer + 2]), y, B, F);
  SDK_LAUNCH_CHECK();
  return 0;
}

template <bool F16>
int head(const char* wb, const sdk_segmentation_desc* d, const float* x, int64_t M, float* logp, hipStream_t st) {
  hipLaunchKernelGGL(seg_head_kernel<F16>, dim3((unsigned)((M + 63) / 64)), dim3(SG_NT), 0, st, x, (int)M,
                     (const bf16_t*)(wb + d->off[SDK_SEG_LIN0_W]), (const float*)(wb + d->off[SDK_SEG_LIN0_B]), (const bf16_t*)(wb + d->off[SDK_SEG_LIN1_W]),
                     (const float*)(wb + d->off[SDK_SEG_LIN1_B]), (const float*)(wb + d->off[SDK_SEG_CLS_W]), (const float*)(wb + d->off[SDK_SEG_CLS_B]), logp);
  SDK_LAUNCH_CHECK();
  return 0;
}

int check_source(const char* fn, const int16_t* samples, int64_t n_samples, int ld, int B, int S) {
  SDK_REQUIRE(S >= 991, "%s: S=%d samples (a chunk needs at least 991 samples for one frame)", fn, S);
  SDK_REQUIRE(B >= 0, "%s: B=%d", fn, B);
  SDK_REQUIRE(samples, "%s: samples is null", fn);
  SDK_REQUIRE(n_samples > 0 && n_samples < (1ll << 31), "%s: n_samples=%lld (1 .. 2^31 - 1)", fn, (long long)n_samples);
  (void)ld;
  return 0;
}

}  // namespace

extern "C" int sdk_segmentation_frames(int S) { return seg_frames(S); }

extern "C" size_t sdk_segmentation_workspace_bytes(const sdk_segmentation_desc* d, int B, int S) {
  if (!d || B <= 0 || S < 991) {
    sdk_set_error("sdk_segmentation_workspace_bytes: d=%p B=%d S=%d (a descriptor, B at least 1, a chunk of at least 991 samples: one frame)", (const void*)d, B, S);
    return 0;
  }
  SegWs w;
  return seg_carve({}, B, S, &w);
}

extern "C" int sdk_sincnet_frontend(sdk_ctx* ctx, const void* wblob, const sdk_segmentation_desc* d, const int16_t* samples, int64_t n_samples,
                                    const int32_t* starts, int ld, int B, int S, void* ws, size_t ws_bytes, float* out, void* stream) {
  if (int rc = check_source("sdk_sincnet_frontend", samples, n_samples, ld, B, S)) return rc;
  SDK_REQUIRE(ctx && wblob && out, "sdk_sincnet_frontend: null argument");
  if (int rc = check_sdesc(d)) return rc;
  if (B == 0) return 0;
  SDK_REQUIRE(starts || (ld >= S && (int64_t)(B - 1) * ld + S <= n_samples),
              "sdk_sincnet_frontend: rows of ld=%d samples: B=%d rows of S=%d need ld >= S and (B - 1) ld + S <= n_samples=%lld", ld, B, S, (long long)n_samples);
  SDK_REQUIRE_WS("sdk_sincnet_frontend", "sdk_segmentation_workspace_bytes", ws, ws_bytes, sdk_segmentation_workspace_bytes(d, B, S), 256);
  SDK_REQUIRE((uintptr_t)wblob % 256 == 0 && (uintptr_t)out % 16 == 0, "sdk_sincnet_frontend: wblob=%p must be 256-byte aligned, out=%p 16-byte aligned", wblob, (void*)out);
  const hipStream_t st = (hipStream_t)stream;
  return d->precision == 2 ? frontend<true>(ctx, (const char*)wblob, d, samples, n_samples, starts, ld, B, S, (char*)ws, out, st)
                           : frontend<false>(ctx, (const char*)wblob, d, samples, n_samples, starts, ld, B, S, (char*)ws, out, st);
}

extern "C" int sdk_bilstm_layer(sdk_ctx* ctx, const void* wblob, const sdk_segmentation_desc* d, int layer, const float* x, int ldx, int B, int F,
                                void* ws, size_t ws_bytes, float* y, void* stream) {
  SDK_REQUIRE(ctx && wblob && x && y, "sdk_bilstm_layer: null argument");
  if (int rc = check_sdesc(d)) return rc;
  SDK_REQUIRE(layer >= 0 && layer < 4, "sdk_bilstm_layer: layer=%d (0 .. 3)", layer);
  SDK_REQUIRE(B >= 0 && F >= 1, "sdk_bilstm_layer: B=%d F=%d", B, F);
  if (B == 0) return 0;
  const int kin = layer ? 256 : 64;
  SDK_REQUIRE(ldx >= kin && ldx % 8 == 0, "sdk_bilstm_layer: ldx=%d (a multiple of 8, at least %d for layer %d)", ldx, kin, layer);
  SDK_REQUIRE((int64_t)B * F < (1ll << 31) / 64, "sdk_bilstm_layer: B*F=%lld frames too many", (long long)B * F);
  SDK_REQUIRE_WS("sdk_bilstm_layer", "4096 B F: the gate pre-activations", ws, ws_bytes, (size_t)B * F * 1024 * 4, 256);
  SDK_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)wblob % 256 == 0,
              "sdk_bilstm_layer: x=%p and y=%p must be 16-byte aligned, wblob=%p 256-byte aligned", (const void*)x, (void*)y, wblob);
  const hipStream_t st = (hipStream_t)stream;
  return d->precision == 2 ? bilstm<true>((const char*)wblob, d, layer, x, ldx, B, F, (float*)ws, y, st)
                           : bilstm<false>((const char*)wblob, d, layer, x, ldx, B, F, (float*)ws, y, st);
}

extern "C" int sdk_segmentation_forward(sdk_ctx* ctx, const void* wblob, const sdk_segmentation_desc* d, const int16_t* samples, int64_t n_samples,
                                        const int32_t* starts, int ld, int B, int S, void* ws, size_t ws_bytes, float* logp, void* stream) {
  if (int rc = check_source("sdk_segmentation_forward", samples, n_samples, ld, B, S)) return rc;
  SDK_REQUIRE(ctx && wblob && logp, "sdk_segmentation_forward: null argument");
  if (int rc = check_sdesc(d)) return rc;
  if (B == 0) return 0;
  SDK_REQUIRE(starts || (ld >= S && (int64_t)(B - 1) * ld + S <= n_samples),
              "sdk_segmentation_forward: rows of ld=%d samples: B=%d rows of S=%d need ld >= S and (B - 1) ld + S <= n_samples=%lld", ld, B, S,
              (long long)n_samples);
  const int F = seg_frames(S);
  SDK_REQUIRE((int64_t)B * F < (1ll << 31) / 64, "sdk_segmentation_forward: B*F=%lld frames too many", (long long)B * F);
  SDK_REQUIRE_WS("sdk_segmentation_forward", "sdk_segmentation_workspace_bytes", ws, ws_bytes, sdk_segmentation_workspace_bytes(d, B, S), 256);
  SDK_REQUIRE((uintptr_t)wblob % 256 == 0, "sdk_segmentation_forward: wblob=%p must be 256-byte aligned", wblob);
  const hipStream_t st = (hipStream_t)stream;
  const char* wb = (const char*)wblob;
  char* w = (char*)ws;
  SegWs sw;
  seg_carve({w, 0}, B, S, &sw);
  float* const X0 = sw.R2;             // the 60-d frames [B F][64] (R2 is free once conv 3 has read its input)
  float *const G = sw.R1, *const H = sw.R3;
  const bool f16 = d->precision == 2;
  // the last norm reads R1 and writes X0 in R2, whose conv-3 input is dead by then
  if (int rc = f16 ? frontend<true>(ctx, wb, d, samples, n_samples, starts, ld, B, S, w, X0, st)
                   : frontend<false>(ctx, wb, d, samples, n_samples, starts, ld, B, S, w, X0, st)) return rc;
  for (int l = 0; l < 4; ++l) {
    const float* in = l ? H : X0;
    if (int rc = f16 ? bilstm<true>(wb, d, l, in, l ? 256 : 64, B, F, G, H, st) : bilstm<false>(wb, d, l, in, l ? 256 : 64, B, F, G, H, st)) return rc;
  }
  return f16 ? head<true>(wb, d, H, (int64_t)B * F, logp, st) : head<false>(wb, d, H, (int64_t)B * F, logp, st);
}
