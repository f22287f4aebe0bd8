// What the model forwards (forward_ecapa.hip, forward_xvector.hip, forward_resnet.hip) build their launch sequences from: the view of a packed
// weight blob, the argument values of the two conv GEMMs, the two GEMMs of the ASP tail and the refusals every family words alike.  Host code
// only, plain aggregates and inline functions: these run some 45 times per forward on the thread that also launches.
#pragma once
#include <string.h>

#include "common.hpp"
#include "ecapa_layout.h"
#include "hp.hpp"

// A packed device weight blob under a descriptor's off[]: slot -> typed pointer, null where the descriptor marks the slot absent (off < 0)
struct Blob {
  const char* base;
  const int64_t* off;
  template <class T>
  const T* at(int slot) const { return off[slot] < 0 ? nullptr : (const T*)(base + off[slot]); }
  const uint16_t* p16(int slot) const { return at<uint16_t>(slot); }
  const float* p32(int slot) const { return at<float>(slot); }
};

// ---- sdk_conv_gemm_args / sdk_conv_gemm_hp_args (G): all zero, then the geometry; the operands by the setters below.  A 2-byte operand of the
// precise mode is a plane pair [rows, ld] whose lo plane lies ld / 2 columns to the right of its hi plane, at every call site of the forwards:
// the hp overloads derive the lo offset.
template <class G>
static inline G gemm_geom(int M, int N, int Cin, int taps, int dil, int T, uint32_t flags) {
  G g;
  memset(&g, 0, sizeof(g));
  g.M = M; g.N = N; g.Cin = Cin; g.taps = taps; g.dil = dil; g.T = T; g.flags = flags;
  return g;
}
static inline void gemm_a(sdk_conv_gemm_args& g, const uint16_t* A, int64_t lda) { g.A = A; g.lda = lda; }
static inline void gemm_a(sdk_conv_gemm_hp_args& g, const uint16_t* A, int64_t lda) { g.A = A; g.lda = lda; g.a_lo = lda >> 1; }
static inline void gemm_c(sdk_conv_gemm_args& g, uint16_t* C, int64_t ldc) { g.C = C; g.ldc = ldc; }
static inline void gemm_c(sdk_conv_gemm_hp_args& g, uint16_t* C, int64_t ldc) { g.C = C; g.ldc = ldc; g.c_lo = ldc >> 1; }
// the second output S = C + X2 (the Res2Net running sum)
static inline void gemm_sum(sdk_conv_gemm_args& g, const uint16_t* X2, int64_t ldx2, uint16_t* S, int64_t lds) { g.X2 = X2; g.ldx2 = ldx2; g.S = S; g.lds = lds; }
static inline void gemm_sum(sdk_conv_gemm_hp_args& g, const uint16_t* X2, int64_t ldx2, uint16_t* S, int64_t lds) {
  g.X2 = X2; g.ldx2 = ldx2; g.x2_lo = ldx2 >> 1; g.S = S; g.lds = lds; g.s_lo = lds >> 1;
}
static inline int gemm_run(sdk_ctx* ctx, const sdk_conv_gemm_args& g, void* stream) { return sdk_conv_gemm(ctx, &g, stream); }
static inline int gemm_run(sdk_ctx* ctx, const sdk_conv_gemm_hp_args& g, void* stream) { return sdk_conv_gemm_hp(ctx, &g, stream); }

// One frame layer, conv -> ReLU (in flags) -> folded BN, on the four blob slots W, bias, scale, shift that start at `slot`: the ECAPA layout's
// slot + EL_W .. EL_SHIFT and the x-vector layout's 4 l + 0 .. 3 are the same order
template <class G>
static inline G gemm_layer(const Blob& b, int slot, const uint16_t* A, int64_t lda, uint16_t* C, int64_t ldc, int M, int N, int Cin, int taps, int dil, int T,
                           uint32_t flags) {
  G g = gemm_geom<G>(M, N, Cin, taps, dil, T, flags);
  gemm_a(g, A, lda);
  gemm_c(g, C, ldc);
  g.W = b.p16(slot + EL_W); g.bias = b.p32(slot + EL_B); g.scale = b.p32(slot + EL_SCALE); g.shift = b.p32(slot + EL_SHIFT);
  return g;
}

// ---- the two GEMMs of the ASP tail (tb: EL_TAIL_BASE of the blob), default / masked forward on sdk_conv_gemm_args, precise on the hp struct
// attention hidden: ah = tanh(BN(relu(W_h h + ubias[segment row]))), the context bias one row of ubias per segment, ldub apart
template <class G>
static inline int asp_hidden_gemm(sdk_ctx* ctx, const Blob& b, int tb, const uint16_t* h, int64_t ldh, uint16_t* ah, int64_t ldah, const float* ubias, int64_t ldub,
                                  int M, int Cm, int A, int T, uint32_t flags, void* stream) {
  G g = gemm_geom<G>(M, A, Cm, 1, 1, T, SDK_GEMM_RELU | SDK_GEMM_TANH | flags);
  gemm_a(g, h, ldh);
  gemm_c(g, ah, ldah);
  g.W = b.p16(tb + EL_ASP_WH); g.ubias = ubias; g.ldub = ldub; g.scale = b.p32(tb + EL_ASP_SCALE); g.shift = b.p32(tb + EL_ASP_SHIFT);
  return gemm_run(ctx, g, stream);
}
// attention logits [M, Cm] in fp32
template <class G>
static inline int asp_logits_gemm(sdk_ctx* ctx, const Blob& b, int tb, const uint16_t* ah, int64_t ldah, float* logits, int M, int Cm, int A, int T, uint32_t flags,
                                  void* stream) {
  G g = gemm_geom<G>(M, Cm, A, 1, 1, T, flags);
  gemm_a(g, ah, ldah);
  g.W = b.p16(tb + EL_ASP_W2); g.C32 = logits; g.ldc32 = Cm; g.bias = b.p32(tb + EL_ASP_B2);
  return gemm_run(ctx, g, stream);
}

// ---- the refusals that the x-vector and ResNet34 entry points word alike, after their own batch and feature-width checks: the workspace (null,
// short, misaligned), then the blob's alignment.  (The ECAPA entry points name no pointer in the latter: check_forward_args keeps its own line.)
static inline int check_ws_and_blob(const char* fn, const char* sizer, const void* ws, size_t ws_bytes, size_t need, const void* wblob) {
  SDK_REQUIRE_WS(fn, sizer, ws, ws_bytes, need, 256);
  SDK_REQUIRE(((uintptr_t)wblob % 256) == 0, "%s: wblob=%p must be 256-byte aligned", fn, wblob);
  return 0;
}
