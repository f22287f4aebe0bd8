// The x-vector forward: the plain TDNN embedding extractor (Snyder et al. 2018) composed from the pieces of the ECAPA forward: every frame layer
// is one sdk_conv_gemm (conv -> ReLU -> folded BN -> bf16), the pooled statistics and the embedding layer are fp32.
#include <type_traits>

#include "forward.hpp"

namespace {
int check_xdesc(const sdk_xvector_desc* d) {
  SDK_REQUIRE(d, "xvector desc is null");
  SDK_REQUIRE(d->n_frame_layers >= 1 && d->n_frame_layers <= 8, "xvector desc: n_frame_layers=%d", d->n_frame_layers);
  SDK_REQUIRE(d->embed_dim > 0 && d->n_feats > 0, "xvector desc: embed_dim=%d n_feats=%d", d->embed_dim, d->n_feats);
  for (int l = 0; l < d->n_frame_layers; ++l) {
    SDK_REQUIRE((d->kernel[l] & 1) == 1 && d->dilation[l] >= 1 && d->cout[l] % 128 == 0 && d->cout[l] > 0, "xvector desc: layer %d kernel=%d dil=%d cout=%d", l,
                d->kernel[l], d->dilation[l], d->cout[l]);
    if (l > 0) SDK_REQUIRE(d->cin[l] == d->cout[l - 1] && d->cin[l] % 64 == 0, "xvector desc: layer %d cin=%d does not follow cout=%d", l, d->cin[l], d->cout[l - 1]);
    for (int q = 0; q < 4; ++q) SDK_REQUIRE(d->off[4 * l + q] >= 0, "xvector desc: slot %d of layer %d missing", q, l);
  }
  SDK_REQUIRE(d->off[62] >= -1 && d->off[62] <= 2, "xvector desc: off[62] (precision of the blob) must be -1 / 0 (bf16 operands), 1 (fp16 hi + lo planes) or 2 (one fp16 plane)");
  if (d->off[62] == 1)
    SDK_REQUIRE(d->cin[0] == d->n_feats && d->n_feats % 32 == 0 && d->first_tap_pack == 0, "xvector desc: a precise-mode blob reads %d feature channels (a multiple of 32, no tap packing)", d->n_feats);
  else
  SDK_REQUIRE(d->cin[0] == d->n_feats && (d->first_tap_pack == 0 ? d->n_feats % 64 == 0 : (d->first_tap_pack == d->n_feats && d->n_feats % 8 == 0 && d->kernel[0] > 1)),
              "xvector desc: first layer over %d features needs them to be a multiple of 64, or its taps packed (first_tap_pack = n_feats, a multiple of 8)", d->n_feats);
  SDK_REQUIRE(d->off[60] >= 0 && d->off[61] >= 0, "xvector desc: embedding layer slots missing");
  return 0;
}
struct XvWs {
  uint16_t *b0, *b1;
  float* stats;
};
size_t xv_carve(WsCarver c, const sdk_xvector_desc* d, int B, int T, XvWs* w) {
  size_t cmax = 0;
  for (int l = 0; l < d->n_frame_layers; ++l) cmax = (size_t)d->cout[l] > cmax ? (size_t)d->cout[l] : cmax;
  const size_t M = (size_t)B * T;
  const size_t planes = d->off[62] == 1 ? 2 : 1;               // precise blob: activations travel as fp16 hi + lo planes (4 bytes per element)
  w->b0 = c.take<uint16_t>(M * cmax * planes);
  w->b1 = c.take<uint16_t>(M * cmax * planes);
  w->stats = c.take<float>((size_t)B * 2 * d->cout[d->n_frame_layers - 1]);
  return c.bytes();
}

// the frame layers on G's GEMM, ping-ponging between the two buffers: feats [M, ldf] -> the last layer's output [M, *ldout] (*last).  planes: 2 where
// an activation is a plane pair (row length 2 cout, the lo plane cout columns to the right), else 1
template <class G>
int xv_frame_layers(sdk_ctx* ctx, const Blob& blob, const sdk_xvector_desc* d, const uint16_t* feats, int ldf, int M, int T, const XvWs& w, int planes,
                    uint32_t flags, const uint16_t** last, int64_t* ldout, void* stream) {
  const uint16_t* in = feats;
  int64_t ldin = ldf;
  for (int l = 0; l < d->n_frame_layers; ++l) {
    uint16_t* out = (l & 1) ? w.b1 : w.b0;
    const int64_t ldo = planes * (int64_t)d->cout[l];
    G g = gemm_layer<G>(blob, 4 * l, in, ldin, out, ldo, M, d->cout[l], d->cin[l], d->kernel[l], d->dilation[l], T, flags);
    if constexpr (std::is_same<G, sdk_conv_gemm_args>::value)      // (the precise GEMM packs no taps: check_xdesc)
      if (l == 0 && d->first_tap_pack) g.tap_pack = d->first_tap_pack;
    if (int rc = gemm_run(ctx, g, stream)) return rc;
    in = out;
    ldin = ldo;
  }
  *last = in;
  *ldout = ldin;
  return 0;
}
}  // namespace

extern "C" size_t sdk_xvector_workspace_bytes(const sdk_xvector_desc* d, int B, int T) {
  if (!d || B <= 0 || T <= 0 || (int64_t)B * T >= (1ll << 31) || d->n_frame_layers < 1 || d->n_frame_layers > 8) {
    sdk_set_error("sdk_xvector_workspace_bytes: d=%p B=%d T=%d n_frame_layers=%d (a descriptor of 1 .. 8 frame layers, B and T at least 1, B*T below 2^31)",
                  (const void*)d, B, T, d ? d->n_frame_layers : -1);
    return 0;
  }
  XvWs w;
  return xv_carve({}, d, B, T, &w);
}

extern "C" int sdk_xvector_forward(sdk_ctx* ctx, const void* wblob, const sdk_xvector_desc* d, const uint16_t* feats, int ldf, int B, int T,
                                   void* ws, size_t ws_bytes, float* emb, void* stream) {
  SDK_REQUIRE(ctx && wblob && feats && ws && emb, "sdk_xvector_forward: null argument");
  if (int rc = check_xdesc(d)) return rc;
  const bool hp = d->off[62] == 1, f16 = d->off[62] == 2;
  // (the blob's precision decides, per call; the features must be in its format: bf16 for 0, fp16 hi | lo planes for 1, one fp16 plane for 2)
  SDK_REQUIRE(B > 0 && T > 0 && (int64_t)B * T < (1ll << 31), "sdk_xvector_forward: bad batch (B=%d T=%d)", B, T);
  if (hp) SDK_REQUIRE(ldf % 16 == 0 && (ldf >> 1) >= d->n_feats && d->first_tap_pack == 0 && d->n_feats % 32 == 0,
                      "sdk_xvector_forward: precise mode reads fp16 planes [B*T, ldf] with the lo plane ldf/2 columns to the right: ldf=%d, n_feats=%d (a multiple of 32, no tap packing)", ldf, d->n_feats);
  else SDK_REQUIRE(ldf >= d->n_feats && ldf % 8 == 0, "sdk_xvector_forward: ldf=%d < feature width %d", ldf, d->n_feats);
  for (int l = 0; l < d->n_frame_layers; ++l)
    SDK_REQUIRE(T > (d->kernel[l] / 2) * d->dilation[l], "sdk_xvector_forward: segments of %d frames are shorter than layer %d's halo", T, l);
  if (int rc = check_ws_and_blob("sdk_xvector_forward", "sdk_xvector_workspace_bytes", ws, ws_bytes, sdk_xvector_workspace_bytes(d, B, T), wblob)) return rc;
  XvWs w;
  xv_carve({(char*)ws, 0}, d, B, T, &w);
  const Blob blob{(const char*)wblob, d->off};
  const int Cl = d->cout[d->n_frame_layers - 1];
  const uint16_t* h;
  int64_t ldh;
  if (hp) {
    // precise mode (north_star's 1e-5): every frame layer on the fp16 hi+lo plane GEMM (three MFMAs per product, csrc/hp.hip), planes between the
    // layers, statistics pooling on the planes; the embedding layer is fp32 either way
    if (int rc = xv_frame_layers<sdk_conv_gemm_hp_args>(ctx, blob, d, feats, ldf, B * T, T, w, 2, SDK_GEMM_RELU, &h, &ldh, stream)) return rc;
    if (int rc = hp_asp_stats(ctx, h, ldh, ldh >> 1, B, T, Cl, w.stats, stream)) return rc;
  } else {
    if (int rc = xv_frame_layers<sdk_conv_gemm_args>(ctx, blob, d, feats, ldf, B * T, T, w, 1, SDK_GEMM_RELU | (f16 ? SDK_GEMM_F16 : 0u), &h, &ldh, stream)) return rc;
    if (int rc = asp_stats_impl(ctx, h, ldh, B, T, Cl, w.stats, stream, f16)) return rc;
  }
  return sdk_rows_fc(ctx, w.stats, 2 * Cl, nullptr, nullptr, blob.p32(60), blob.p32(61), emb, d->embed_dim, B, 2 * Cl, d->embed_dim, 0, stream);
}
