// The ResNet34 forwards, plain and masked: the WeSpeaker ResNet34 (the PyAnnote 3.1 speaker embedding): one sdk_resnet_conv2d per conv (a
// downsampling block's projection shortcut rides in its conv2's K), the temporal statistics pooling, and the embedding layer on sdk_rows_fc (fp32).
#include "forward.hpp"

namespace {
int check_rdesc(const sdk_resnet_desc* d) {
  SDK_REQUIRE(d, "resnet desc is null");
  SDK_REQUIRE(d->precision != 1, "resnet desc: precision 1 (the precise mode, SDK_PRECISION=1) is not built for the ResNet34 family; use 0 (bf16) or 2 (fp16)");
  SDK_REQUIRE(d->precision == 0 || d->precision == 2, "resnet desc: precision=%d (0: bf16 operands, 2: one fp16 plane)", d->precision);
  SDK_REQUIRE(d->n_layers == 4 && d->n_feats > 0 && d->embed_dim > 0, "resnet desc: n_layers=%d n_feats=%d embed_dim=%d", d->n_layers, d->n_feats, d->embed_dim);
  SDK_REQUIRE(d->width[0] == 32, "resnet desc: width[0]=%d (the stem writes 32 channels)", d->width[0]);
  int nconv = 1;
  for (int l = 0; l < 4; ++l) {
    SDK_REQUIRE(d->blocks[l] >= 1 && d->blocks[l] <= 8, "resnet desc: blocks[%d]=%d", l, d->blocks[l]);
    SDK_REQUIRE(d->width[l] == 32 || d->width[l] == 64 || d->width[l] == 128 || d->width[l] == 256, "resnet desc: width[%d]=%d", l, d->width[l]);
    nconv += 2 * d->blocks[l];
  }
  SDK_REQUIRE(nconv <= 33, "resnet desc: %d convs (at most 33 slots)", nconv);
  for (int i = 0; i < 2 * nconv; ++i) SDK_REQUIRE(d->off[i] >= 0 && d->off[i] % 256 == 0, "resnet desc: slot %d missing or misaligned", i);
  SDK_REQUIRE(d->off[66] >= 0 && d->off[67] >= 0 && d->off[66] % 256 == 0 && d->off[67] % 256 == 0, "resnet desc: seg_1 slots missing");
  return 0;
}
int rn_out(int n, int s) { return (n - 1) / s + 1; }
// the three activation buffers hold the largest map of the network; then the pooled statistics [rows B][2 C4 F4] (rows = 1: one per segment;
// the masked forward has S per segment)
struct RnWs {
  uint16_t* buf[3];
  float* stats;
};
size_t rn_carve(WsCarver c, const sdk_resnet_desc* d, int B, int T, int rows, RnWs* w) {
  int F = d->n_feats, Tl = T;
  size_t big = (size_t)F * T * d->width[0];
  for (int l = 0; l < 4; ++l) {
    if (l) { F = rn_out(F, 2); Tl = rn_out(Tl, 2); }
    const size_t e = (size_t)F * Tl * d->width[l];
    big = e > big ? e : big;
  }
  for (int i = 0; i < 3; ++i) w->buf[i] = c.take<uint16_t>((size_t)B * big);
  w->stats = c.take<float>((size_t)B * rows * 2 * d->width[3] * F);
  return c.bytes();
}

// the conv trunk shared by both forwards: feats -> the last map [B][F][Tl][C] in one of the three buffers (*last)
int rn_trunk(sdk_ctx* ctx, const Blob& blob, const sdk_resnet_desc* d, const uint16_t* feats, int ldf, int B, int T, uint16_t* const* buf,
             const uint16_t** last, int* Fl, int* Tlast, int* Cl, void* stream) {
  const uint32_t fl = SDK_GEMM_RELU | (d->precision == 2 ? SDK_GEMM_F16 : 0u);
  // conv i of the blob (weights at slot 2 i, bias at 2 i + 1) from x [B][F][Tx][Cin] to y, everything else zero
  auto conv_args = [&](int i, const uint16_t* x, uint16_t* y, int F, int Tx, int Cin, int Cout, int stride) {
    sdk_resnet_conv_args a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.W = blob.p16(2 * i); a.bias = blob.p32(2 * i + 1); a.y = y;
    a.B = B; a.F = F; a.T = Tx; a.Cin = Cin; a.Cout = Cout; a.stride = stride; a.flags = fl;
    return a;
  };
  uint16_t *X = buf[0], *H = buf[1], *Y = buf[2];
  sdk_resnet_conv_args a = conv_args(0, feats, X, d->n_feats, T, 1, d->width[0], 1);   // the stem reads the fbank matrix [B T, ldf]
  a.ldx = ldf;
  if (int rc = sdk_resnet_conv2d(ctx, &a, stream)) return rc;
  int F = d->n_feats, Tl = T, C = d->width[0], conv = 1;
  for (int l = 0; l < 4; ++l) {
    for (int j = 0; j < d->blocks[l]; ++j) {
      const int s = (j == 0 && l > 0) ? 2 : 1, Cw = d->width[l];
      const int Fo = rn_out(F, s), To = rn_out(Tl, s);
      const bool proj = j == 0 && (s != 1 || C != Cw);
      a = conv_args(conv, X, H, F, Tl, C, Cw, s);                 // conv1 -> BN -> ReLU
      if (int rc = sdk_resnet_conv2d(ctx, &a, stream)) return rc;
      a = conv_args(conv + 1, H, Y, Fo, To, Cw, Cw, 1);           // conv2 -> BN (+ projection shortcut in K | + identity) -> ReLU
      if (proj) { a.sc = X; a.Csc = C; a.Fsc = F; a.Tsc = Tl; a.stride_sc = s; }
      else a.res = X;
      if (int rc = sdk_resnet_conv2d(ctx, &a, stream)) return rc;
      uint16_t* t = X; X = Y; Y = t;
      F = Fo; Tl = To; C = Cw; conv += 2;
    }
  }
  *last = X; *Fl = F; *Tlast = Tl; *Cl = C;
  return 0;
}
}  // namespace

extern "C" size_t sdk_resnet_workspace_bytes(const sdk_resnet_desc* d, int B, int T) {
  if (!d || B <= 0 || T <= 0 || (int64_t)B * T >= (1ll << 31) || d->n_feats <= 0) {
    sdk_set_error("sdk_resnet_workspace_bytes: d=%p B=%d T=%d n_feats=%d (a descriptor, B, T and n_feats at least 1, B*T below 2^31)", (const void*)d, B, T,
                  d ? d->n_feats : -1);
    return 0;
  }
  RnWs w;
  return rn_carve({}, d, B, T, 1, &w);
}

extern "C" size_t sdk_resnet_masked_workspace_bytes(const sdk_resnet_desc* d, int B, int T, int S) {
  if (!d || B <= 0 || T <= 0 || S <= 0 || (int64_t)B * T >= (1ll << 31) || (int64_t)B * S >= (1ll << 31) || d->n_feats <= 0) {
    sdk_set_error("sdk_resnet_masked_workspace_bytes: d=%p B=%d T=%d S=%d n_feats=%d (a descriptor, B, T, S and n_feats at least 1, B*T and B*S below 2^31)",
                  (const void*)d, B, T, S, d ? d->n_feats : -1);
    return 0;
  }
  RnWs w;
  return rn_carve({}, d, B, T, S, &w);
}

extern "C" int sdk_resnet_last_map_frames(const sdk_resnet_desc* d, int T) {
  if (!d || T <= 0) return 0;
  for (int l = 1; l < 4; ++l) T = rn_out(T, 2);
  return T;
}

extern "C" int sdk_resnet_forward(sdk_ctx* ctx, const void* wblob, const sdk_resnet_desc* d, const uint16_t* feats, int ldf, int B, int T,
                                  void* ws, size_t ws_bytes, float* emb, void* stream) {
  SDK_REQUIRE(ctx && wblob && feats && ws && emb, "sdk_resnet_forward: null argument");
  if (int rc = check_rdesc(d)) return rc;
  SDK_REQUIRE(B > 0 && T >= 9 && (int64_t)B * T < (1ll << 31), "sdk_resnet_forward: bad batch (B=%d T=%d; segments need >= 9 frames)", B, T);
  SDK_REQUIRE(ldf >= d->n_feats, "sdk_resnet_forward: ldf=%d < feature width %d", ldf, d->n_feats);
  if (int rc = check_ws_and_blob("sdk_resnet_forward", "sdk_resnet_workspace_bytes", ws, ws_bytes, sdk_resnet_workspace_bytes(d, B, T), wblob)) return rc;
  RnWs rw;
  rn_carve({(char*)ws, 0}, d, B, T, 1, &rw);
  const Blob blob{(const char*)wblob, d->off};
  const uint16_t* X;
  int F, Tl, C;
  if (int rc = rn_trunk(ctx, blob, d, feats, ldf, B, T, rw.buf, &X, &F, &Tl, &C, stream)) return rc;
  if (int rc = resnet_tstp_impl(ctx, X, B, F, Tl, C, rw.stats, stream, d->precision == 2)) return rc;
  return sdk_rows_fc(ctx, rw.stats, 2 * C * F, nullptr, nullptr, blob.p32(66), blob.p32(67), emb, d->embed_dim, B, 2 * C * F, d->embed_dim, 0, stream);
}

extern "C" int sdk_resnet_forward_masked(sdk_ctx* ctx, const void* wblob, const sdk_resnet_desc* d, const uint16_t* feats, int ldf, int B, int T,
                                         int S, const float* w, const int32_t* valid, void* ws, size_t ws_bytes, float* emb, void* stream) {
  SDK_REQUIRE(ctx && wblob && feats && w && valid && ws && emb, "sdk_resnet_forward_masked: null argument");
  if (int rc = check_rdesc(d)) return rc;
  SDK_REQUIRE(B > 0 && T >= 9 && (int64_t)B * T < (1ll << 31), "sdk_resnet_forward_masked: bad batch (B=%d T=%d; segments need >= 9 frames)", B, T);
  SDK_REQUIRE(S >= 1 && (int64_t)B * S < (1ll << 31), "sdk_resnet_forward_masked: S=%d weight rows per segment (B=%d)", S, B);
  SDK_REQUIRE(ldf >= d->n_feats, "sdk_resnet_forward_masked: ldf=%d < feature width %d", ldf, d->n_feats);
  if (int rc = check_ws_and_blob("sdk_resnet_forward_masked", "sdk_resnet_masked_workspace_bytes", ws, ws_bytes, sdk_resnet_masked_workspace_bytes(d, B, T, S), wblob)) return rc;
  RnWs rw;
  rn_carve({(char*)ws, 0}, d, B, T, S, &rw);
  const Blob blob{(const char*)wblob, d->off};
  const uint16_t* X;
  int F, Tl, C;
  if (int rc = rn_trunk(ctx, blob, d, feats, ldf, B, T, rw.buf, &X, &F, &Tl, &C, stream)) return rc;
  if (int rc = resnet_masked_tstp_impl(ctx, X, B, F, Tl, C, S, w, valid, rw.stats, stream, d->precision == 2)) return rc;
  if (int rc = sdk_rows_fc(ctx, rw.stats, 2 * C * F, nullptr, nullptr, blob.p32(66), blob.p32(67), emb, d->embed_dim, B * S, 2 * C * F, d->embed_dim, 0, stream)) return rc;
  return resnet_zero_invalid_impl(ctx, emb, B * S, d->embed_dim, valid, stream);
}
