// The ECAPA-TDNN forward schedules: default / fp16 (sdk_ecapa_forward, sdk_ecapa_forward_calib), precise hi+lo planes, and masked
// (sdk_ecapa_forward_masked).  One C call per batch of segments; every step is an asynchronous launch on the caller's stream, so the whole
// forward can be captured in a hipGraph by the host.
#include "forward.hpp"

namespace {

struct FwdWs {
  uint16_t *X0, *U, *R, *Z, *Sa, *Sb, *CAT, *H, *AH;
  float *ctx, *ubias, *logits, *pooled, *se, *stats, *mean;
};

// full_logits: the masked forward's pooling reads the fp32 logits from HBM at every T
size_t fwd_carve(WsCarver c, const sdk_ecapa_desc* d, int B, int T, FwdWs* w, bool full_logits = false) {
  const size_t M = (size_t)B * T, C = d->channels, Cm = d->mfa_channels, S = d->sub_channels, A = d->attn_channels;
  w->X0 = c.take<uint16_t>(M * C);
  w->U = c.take<uint16_t>(M * C);
  w->R = c.take<uint16_t>(M * C);
  w->Z = c.take<uint16_t>(M * C);
  w->Sa = c.take<uint16_t>(M * S);
  w->Sb = c.take<uint16_t>(M * S);
  w->CAT = c.take<uint16_t>(M * Cm);
  w->H = c.take<uint16_t>(M * Cm);
  w->AH = c.take<uint16_t>(M * A);
  w->ctx = c.take<float>((size_t)B * 2 * Cm);
  w->ubias = c.take<float>((size_t)B * A);
  // the [M, Cm] fp32 attention logits exist in HBM only on the unfused pooling path (37 % of the workspace otherwise)
  const bool fused_asp = !full_logits && A == 128 && T <= sdk_asp_fused_max_frames();
  w->logits = c.take<float>(fused_asp ? 64 : M * Cm);
  w->pooled = c.take<float>((size_t)B * 2 * Cm);
  w->se = (float*)c.take<char>(sdk_se_workspace_bytes(B, (int)C, d->se_channels));
  w->stats = (float*)c.take<char>(sdk_conv_gemm_stats_bytes((int)M, (int)Cm, 2));
  w->mean = c.take<float>((size_t)B * C);
  return c.bytes();
}

// ---- precise mode: every activation a pair of fp16 planes [M, 2 C] (hi | lo), logits fp32
struct FwdWsHp {
  uint16_t *X0, *U, *R, *Z, *Sa, *Sb, *CAT, *H, *AH;
  float *ctx, *ubias, *logits, *pooled, *mean, *hid, *gate;
};

size_t fwd_carve_hp(WsCarver c, const sdk_ecapa_desc* d, int B, int T, FwdWsHp* w) {
  const size_t M = (size_t)B * T, C = d->channels, Cm = d->mfa_channels, S = d->sub_channels, A = d->attn_channels;
  w->X0 = c.take<uint16_t>(M * C * 2);
  w->U = c.take<uint16_t>(M * C * 2);
  w->R = c.take<uint16_t>(M * C * 2);
  w->Z = c.take<uint16_t>(M * C * 2);
  w->Sa = c.take<uint16_t>(M * S * 2);
  w->Sb = c.take<uint16_t>(M * S * 2);
  w->CAT = c.take<uint16_t>(M * Cm * 2);
  w->H = c.take<uint16_t>(M * Cm * 2);
  w->AH = c.take<uint16_t>(M * A * 2);
  w->ctx = c.take<float>((size_t)B * 2 * Cm);
  w->ubias = c.take<float>((size_t)B * A);
  w->logits = c.take<float>(M * Cm);
  w->pooled = c.take<float>((size_t)B * 2 * Cm);
  w->mean = c.take<float>((size_t)B * C);
  w->hid = c.take<float>((size_t)B * d->se_channels);
  w->gate = c.take<float>((size_t)B * C);
  return c.bytes();
}

int check_desc(const sdk_ecapa_desc* d) {
  SDK_REQUIRE(d, "ecapa desc is null");
  SDK_REQUIRE(d->n_blocks >= 1 && d->n_blocks <= 4, "ecapa desc: n_blocks=%d", d->n_blocks);
  SDK_REQUIRE(d->channels % 128 == 0 && d->mfa_channels == d->n_blocks * d->channels, "ecapa desc: channels=%d mfa=%d", d->channels, d->mfa_channels);
  SDK_REQUIRE(d->scale >= 2 && d->sub_channels * d->scale == d->channels && d->sub_channels % 128 == 0, "ecapa desc: res2net scale=%d sub=%d", d->scale, d->sub_channels);
  SDK_REQUIRE(d->attn_channels % 128 == 0 && d->n_mels_padded % (d->precision == 1 ? 32 : 64) == 0, "ecapa desc: attn=%d mels=%d", d->attn_channels, d->n_mels_padded);
  SDK_REQUIRE((d->kernel0 & 1) == 1, "ecapa desc: kernel0=%d must be odd", d->kernel0);
  SDK_REQUIRE(d->precision >= 0 && d->precision <= 2, "ecapa desc: precision=%d", d->precision);
  return 0;
}

// The forward in precise mode (hp.hip): the same layer sequence on fp16 hi+lo planes, every GEMM as three fp16 MFMAs per product,
// no fusion (the Res2Net chain as seven launches with the running sum in the epilogue, SE as mean sweep + two FCs + apply sweep,
// attention logits in fp32 through HBM): this mode buys accuracy, the default mode is the fast one.  A plane pair of width X is (pointer, 2 X):
// the lo plane X columns to the right.
int ecapa_forward_hp(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf, int B, int T, void* ws,
                     float* emb, void* stream) {
  typedef sdk_conv_gemm_hp_args G;
  FwdWsHp w;
  fwd_carve_hp({(char*)ws, 0}, d, B, T, &w);
  const Blob blob{(const char*)wblob, d->off};
  const int M = B * T, C = d->channels, Cm = d->mfa_channels, S = d->sub_channels, A = d->attn_channels, Cse = d->se_channels;
  SDK_REQUIRE(ldf % 16 == 0 && (ldf >> 1) >= d->n_mels_padded, "sdk_ecapa_forward: precise mode takes feature planes, ldf=%d must be >= 2 x %d", ldf, d->n_mels_padded);

  auto tdnn = [&](const uint16_t* Ain, int64_t lda, int Cin, int taps, int dil, int slot, int N, uint16_t* Cout, int64_t ldc, const uint16_t* X2 = nullptr,
                  int64_t ldx2 = 0, uint16_t* Sout = nullptr, int64_t lds = 0) -> int {
    G g = gemm_layer<G>(blob, slot, Ain, lda, Cout, ldc, M, N, Cin, taps, dil, T, SDK_GEMM_RELU);
    gemm_sum(g, X2, ldx2, Sout, lds);
    SDK_REQUIRE(g.W && g.bias && g.scale && g.shift, "sdk_ecapa_forward: weight slot %d missing", slot);
    return gemm_run(ctx, g, stream);
  };
  hipStream_t st = (hipStream_t)stream;

  if (int rc = tdnn(feats, ldf, d->n_mels_padded, d->kernel0, 1, EL_BLK0, C, w.X0, 2 * C)) return rc;
  const uint16_t* xin = w.X0;
  int64_t ldx = 2 * C;
  for (int i = 1; i <= d->n_blocks; ++i) {
    const int base = EL_BLOCK_BASE(i), dil = d->dilation[i - 1];
    if (int rc = tdnn(xin, ldx, C, 1, 1, base + EL_TDNN1, C, w.U, 2 * C)) return rc;
    {   // Res2Net chunk 0 passes through: both planes
      ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 2.0 * M * S * 4);
      SDK_HIP_OK(hipMemcpy2DAsync(w.R, (size_t)C * 4, w.U, (size_t)C * 4, (size_t)S * 2, (size_t)M, hipMemcpyDeviceToDevice, st));
      SDK_HIP_OK(hipMemcpy2DAsync(w.R + C, (size_t)C * 4, w.U + C, (size_t)C * 4, (size_t)S * 2, (size_t)M, hipMemcpyDeviceToDevice, st));
    }
    for (int j = 0; j < d->scale - 1; ++j) {
      const uint16_t* Ain = j == 0 ? w.U + S : ((j & 1) ? w.Sa : w.Sb);
      const int64_t lda = j == 0 ? 2 * C : 2 * S;
      const bool more = j + 1 < d->scale - 1;
      uint16_t* Sout = more ? ((j & 1) ? w.Sb : w.Sa) : nullptr;
      const uint16_t* X2 = more ? w.U + (int64_t)S * (j + 2) : nullptr;
      if (int rc = tdnn(Ain, lda, S, 3, dil, base + EL_RES2NET(j), S, w.R + (int64_t)S * (j + 1), 2 * C, X2, 2 * C, Sout, 2 * S)) return rc;
    }
    if (int rc = tdnn(w.R, 2 * C, C, 1, 1, base + EL_TDNN2, C, w.Z, 2 * C)) return rc;
    // squeeze-excitation: mean sweep, two per-utterance FCs (fp32 matrix pipe), apply sweep
    if (int rc = hp_seg_mean(ctx, w.Z, 2 * C, C, B, T, C, w.mean, stream)) return rc;
    if (int rc = sdk_rows_fc(ctx, w.mean, C, nullptr, nullptr, blob.p32(base + EL_SE_W1T), blob.p32(base + EL_SE_B1), w.hid, Cse, B, C, Cse, 1, stream)) return rc;
    if (int rc = sdk_rows_fc(ctx, w.hid, Cse, nullptr, nullptr, blob.p32(base + EL_SE_W2T), blob.p32(base + EL_SE_B2), w.gate, C, B, Cse, C, 2, stream)) return rc;
    uint16_t* slab = w.CAT + (int64_t)C * (i - 1);
    if (int rc = hp_se_apply(ctx, w.Z, 2 * C, C, xin, ldx, ldx >> 1, w.gate, slab, 2 * Cm, Cm, B, T, C, stream)) return rc;
    xin = slab;
    ldx = 2 * Cm;
  }
  const int tb = EL_TAIL_BASE(d->n_blocks);
  if (int rc = tdnn(w.CAT, 2 * Cm, Cm, 1, 1, tb + EL_MFA, Cm, w.H, 2 * Cm)) return rc;
  if (int rc = hp_asp_stats(ctx, w.H, 2 * Cm, Cm, B, T, Cm, w.ctx, stream)) return rc;
  if (int rc = sdk_rows_fc(ctx, w.ctx, 2 * Cm, nullptr, nullptr, blob.p32(tb + EL_ASP_WMS_T), blob.p32(tb + EL_ASP_B), w.ubias, A, B, 2 * Cm, A, 0, stream)) return rc;
  if (int rc = asp_hidden_gemm<G>(ctx, blob, tb, w.H, 2 * Cm, w.AH, 2 * A, w.ubias, A, M, Cm, A, T, 0, stream)) return rc;
  if (int rc = asp_logits_gemm<G>(ctx, blob, tb, w.AH, 2 * A, w.logits, M, Cm, A, T, 0, stream)) return rc;
  if (int rc = hp_asp_pool(ctx, w.logits, Cm, w.H, 2 * Cm, Cm, B, T, Cm, w.pooled, stream)) return rc;
  return sdk_rows_fc(ctx, w.pooled, 2 * Cm, blob.p32(tb + EL_ASPBN_SCALE), blob.p32(tb + EL_ASPBN_SHIFT), blob.p32(tb + EL_FC_WT), blob.p32(tb + EL_FC_B), emb,
                     d->embed_dim, B, 2 * Cm, d->embed_dim, 0, stream);
}

// Calibration slots (sdk_ecapa_forward_calib): per-segment mean | std (sdk_asp_stats layout [B, 2 C_l]) of the INPUT of every bf16 GEMM layer whose
// weight rounding the host corrects in the bias (weights_pack.bias_corrections): per block tdnn1, the Res2Net convs, tdnn2; then MFA, ASP hidden.
size_t calib_offset(const sdk_ecapa_desc* d, int B, int block, int layer) {   // block < n_blocks: layer 0 = tdnn1, 1..scale-1 = Res2Net conv
  const size_t C = d->channels, S = d->sub_channels, Cm = d->mfa_channels, nr = d->scale - 1;   // layer - 1, scale = tdnn2; block == n_blocks: 0 = MFA,
  const size_t per_block = 2 * C + nr * 2 * S + 2 * C;                                            // 1 = ASP hidden, 2 = end
  size_t off;
  if (block < d->n_blocks) {
    off = (size_t)block * per_block;
    if (layer >= 1) off += 2 * C + (size_t)(layer - 1) * 2 * S;        // (layer == scale: behind the nr Res2Net slots)
  } else {
    off = (size_t)d->n_blocks * per_block + (size_t)layer * 2 * Cm;
  }
  return off * (size_t)B;
}

// The trunk shared by sdk_ecapa_forward and sdk_ecapa_forward_masked: blk0, the SE-Res2Net blocks and MFA, feats -> h [M, Cm] in w.H (K-blocked
// where *h_kb), with the fused column statistics of h in w.stats where *fuse_ctx.  One function, so that the masked forward's h is the
// unmasked forward's bit for bit at the same (B, T): the same launches with the same arguments.  allow_kblocked = false only changes where
// the MFA epilogue stores a value, not the value - on the default GEMM dispatch.  ONE EXCEPTION, reachable through the A/B knob alone: with
// "gemm_variant" 1 (SDK_GEMM_VARIANT=1: every GEMM on the 128^2 kernel) a K-blocked output still forces the 256^2 kernel (sdk_conv_gemm), so
// where the unmasked forward writes h K-blocked (96 < T <= 208 by default) its MFA runs another kernel than the masked forward's and h agrees
// to fp32 summation order only.  At diarization's T = 1001 neither forward writes h K-blocked, whatever the knob.
int ecapa_trunk(sdk_ctx* ctx, const Blob& blob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf, int B, int T, const FwdWs& w, float* calib,
                void* stream, bool allow_kblocked, bool* fuse_ctx_out, bool* h_kb_out) {
  typedef sdk_conv_gemm_args G;
  const int M = B * T, C = d->channels, Cm = d->mfa_channels, S = d->sub_channels, A = d->attn_channels;
  hipStream_t st = (hipStream_t)stream;
  // precision 2 (round 5): the same schedule with every 2-byte tensor - features, weights, activations - in fp16 instead of bf16 (11 significand
  // bits: 7 x closer to the fp32 model at one MFMA per product, profiles/r05_fp16_decision.txt); every stage takes the
  // format per call: the GEMMs from their flag, the sweeps and the two fused launches from an argument of their internal entry
  const bool f16 = d->precision == 2;
  const uint32_t fmt = f16 ? SDK_GEMM_F16 : 0u;

  auto tdnn = [&](const uint16_t* Ain, int64_t lda, int Cin, int taps, int dil, int slot, int N, uint16_t* Cout, int64_t ldc, const uint16_t* X2 = nullptr,
                  int64_t ldx2 = 0, uint16_t* Sout = nullptr, int64_t lds = 0, int stats_mode = 0, uint32_t layout = 0) -> int {
    G g = gemm_layer<G>(blob, slot, Ain, lda, Cout, ldc, M, N, Cin, taps, dil, T, SDK_GEMM_RELU | layout | fmt);
    gemm_sum(g, X2, ldx2, Sout, lds);
    g.stats_mode = stats_mode; g.stats_part = stats_mode ? w.stats : nullptr;
    SDK_REQUIRE(g.W && g.bias && g.scale && g.shift, "sdk_ecapa_forward: weight slot %d missing", slot);
    return gemm_run(ctx, g, stream);
  };
  // the statistics of one calibration slot, on the calibration forward only
  auto calib_stats = [&](const uint16_t* x, int64_t ldx, int Cx, int block, int layer) -> int {
    return calib ? asp_stats_impl(ctx, x, ldx, B, T, Cx, calib + calib_offset(d, B, block, layer), stream, f16) : 0;
  };

  // blk0: k5 conv over the mel channels; with a packed weight slot the five taps share K (5 x 80 -> 448: 7 K-steps instead of 10)
  if (d->blk0_tap_pack > 0) {
    G g = gemm_layer<G>(blob, EL_BLK0, feats, ldf, w.X0, C, M, C, d->blk0_tap_pack, d->kernel0, 1, T, SDK_GEMM_RELU | fmt);
    g.tap_pack = d->blk0_tap_pack;
    SDK_REQUIRE(g.W && g.bias && g.scale && g.shift && d->blk0_tap_pack <= ldf, "sdk_ecapa_forward: blk0 weight slots missing or tap_pack > ldf");
    if (int rc = gemm_run(ctx, g, stream)) return rc;
  } else if (int rc = tdnn(feats, ldf, d->n_mels_padded, d->kernel0, 1, EL_BLK0, C, w.X0, C)) return rc;

  const uint16_t* xin = w.X0;
  int64_t ldx = C;
  for (int i = 1; i <= d->n_blocks; ++i) {
    const int base = EL_BLOCK_BASE(i), dil = d->dilation[i - 1];
    if (int rc = calib_stats(xin, ldx, C, i - 1, 0)) return rc;
    if (int rc = tdnn(xin, ldx, C, 1, 1, base + EL_TDNN1, C, w.U, C)) return rc;
    // Res2Net: chunk 0 passes through, chunk c>=1 = TDNN(chunk c + y_{c-1})
    const uint16_t* r2out = w.R;
    if (S == 128 && d->scale - 1 <= 7 && T <= sdk_res2net_chain_max_frames() && !ctx->no_chain_fusion && !calib) {
      // the seven dependent convolutions in ONE launch, the running tile resident in LDS per segment.  The chain runs
      // IN PLACE on the tdnn1 output: a workgroup has read u_c (into LDS / registers) before it writes y_c over it, and
      // segments do not overlap - so chunk 0 needs no copy
      const uint16_t* Wp[7]; const uint16_t* Wk[7]; const float* bp[7]; const float* sp[7]; const float* tp[7];
      for (int j = 0; j < d->scale - 1; ++j) {
        const int slot = base + EL_RES2NET(j);
        Wp[j] = blob.p16(slot + EL_W); bp[j] = blob.p32(slot + EL_B); sp[j] = blob.p32(slot + EL_SCALE); tp[j] = blob.p32(slot + EL_SHIFT);
        Wk[j] = i <= 4 ? blob.p16(EL_CHAINPACK(i, j)) : nullptr;   // optional fragment-ordered copy
      }
      if (int rc = res2net_chain_launch(ctx, w.U, C, w.U, C, Wp, Wk, bp, sp, tp, d->scale - 1, B, T, dil, stream, f16)) return rc;
      r2out = w.U;
    } else {
      // separate launches: the running sum is produced by the previous conv's epilogue (S output), ping-ponging
      // between two [M, S] buffers
      {
        ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 2.0 * M * S * 2);
        SDK_HIP_OK(hipMemcpy2DAsync(w.R, (size_t)C * 2, w.U, (size_t)C * 2, (size_t)S * 2, (size_t)M, hipMemcpyDeviceToDevice, st));
      }
      for (int j = 0; j < d->scale - 1; ++j) {
        const uint16_t* Ain = j == 0 ? w.U + S : ((j & 1) ? w.Sa : w.Sb);
        const int64_t lda = j == 0 ? C : S;
        const bool more = j + 1 < d->scale - 1;
        uint16_t* Sout = more ? ((j & 1) ? w.Sb : w.Sa) : nullptr;
        const uint16_t* X2 = more ? w.U + (int64_t)S * (j + 2) : nullptr;
        if (int rc = calib_stats(Ain, lda, S, i - 1, 1 + j)) return rc;
        if (int rc = tdnn(Ain, lda, S, 3, dil, base + EL_RES2NET(j), S, w.R + (int64_t)S * (j + 1), C, X2, C, Sout, S)) return rc;
      }
    }
    if (int rc = calib_stats(r2out, C, C, i - 1, d->scale)) return rc;
    // the SE squeeze (per-segment channel means of z) comes out of the tdnn2 epilogue where the shape allows it
    const bool fuse_se = sdk_conv_gemm_stats_fusable(M, C, T) != 0;
    if (int rc = tdnn(r2out, C, C, 1, 1, base + EL_TDNN2, C, w.Z, C, nullptr, 0, nullptr, 0, fuse_se ? 1 : 0)) return rc;
    if (fuse_se)
      if (int rc = sdk_colstats_finish(ctx, w.stats, M, C, T, 1, w.mean, stream)) return rc;
    uint16_t* slab = w.CAT + (int64_t)C * (i - 1);
    if (int rc = se_gate_residual_impl(ctx, w.Z, C, xin, ldx, blob.p32(base + EL_SE_W1T), blob.p32(base + EL_SE_B1), blob.p32(base + EL_SE_W2T),
                                       blob.p32(base + EL_SE_B2), slab, Cm, B, T, C, d->se_channels, fuse_se ? w.mean : nullptr, w.se,
                                       sdk_se_workspace_bytes(B, C, d->se_channels), stream, f16)) return rc;
    xin = slab;
    ldx = Cm;
  }

  const int tb = EL_TAIL_BASE(d->n_blocks);
  // attentive statistics pooling with global context; the context (mean | std of h over frames) comes out of
  // the MFA epilogue where the shape allows it, else from a separate sweep of h
  const bool fuse_ctx = sdk_conv_gemm_stats_fusable(M, Cm, T) != 0;
  if (int rc = calib_stats(w.CAT, Cm, Cm, d->n_blocks, 0)) return rc;
  // h [M, Cm] is the widest activation and is read twice, both times in 64- / 32-channel pieces of its 6-KB rows (the skinny attention-hidden GEMM,
  // the per-segment ASP slabs): where those two are its only readers it is written K-BLOCKED, [Cm / 64][M][64] (sdk_hip.h SDK_GEMM_C_KBLOCKED)
  const bool h_kb = allow_kblocked && !ctx->no_h_kblocked && !calib && fuse_ctx && A == 128 && sdk_asp_kblocked_ok(ctx, T, Cm) != 0;
  if (int rc = tdnn(w.CAT, Cm, Cm, 1, 1, tb + EL_MFA, Cm, w.H, Cm, nullptr, 0, nullptr, 0, fuse_ctx ? 2 : 0, h_kb ? SDK_GEMM_C_KBLOCKED : 0)) return rc;
  if (int rc = calib_stats(w.H, Cm, Cm, d->n_blocks, 1)) return rc;
  *fuse_ctx_out = fuse_ctx;
  *h_kb_out = h_kb;
  return 0;
}

// The checks both forwards make after their null-pointer and descriptor checks, in sdk_ecapa_forward's order and words (fn: the entry point's name;
// need: its workspace size): batch, feature width, receptive halo, workspace, alignment, weight slots.
int check_forward_args(const char* fn, const void* wblob, const sdk_ecapa_desc* d, int ldf, int B, int T, const void* ws, size_t ws_bytes, const char* sizer, size_t need) {
  SDK_REQUIRE(B > 0 && T > 0, "%s: empty batch (B=%d T=%d)", fn, B, T);
  SDK_REQUIRE((int64_t)B * T < (1ll << 31), "%s: B*T overflows int32; split the batch", fn);
  SDK_REQUIRE(ldf >= d->n_mels_padded && ldf % 8 == 0, "%s: ldf=%d < padded mel width %d", fn, ldf, d->n_mels_padded);
  // The numerical contract is the DESCRIPTOR's (per call): features must be in that format (sdk_fbank_fmt with the same precision).  The context's
  // "precision" option plays no part here since round 5 - two engines with different contracts on one device share no mutable state.
  int maxhalo = d->kernel0 / 2;
  for (int i = 0; i < d->n_blocks; ++i) maxhalo = d->dilation[i] > maxhalo ? d->dilation[i] : maxhalo;
  SDK_REQUIRE(T > maxhalo, "%s: segments of %d frames are shorter than the receptive halo %d", fn, T, maxhalo);
  SDK_REQUIRE_WS(fn, sizer, ws, ws_bytes, need, 256);
  SDK_REQUIRE(((uintptr_t)wblob % 256) == 0, "%s: wblob must be 256-byte aligned", fn);

  {  // every slot the schedule dereferences must be present in the blob
    const int tbs = EL_TAIL_BASE(d->n_blocks);
    for (int i = 1; i <= d->n_blocks; ++i)
      for (int s = EL_SE_W1T; s <= EL_SE_B2; ++s)
        SDK_REQUIRE(d->off[EL_BLOCK_BASE(i) + s] >= 0, "%s: SE weight slot %d of block %d missing", fn, s, i);
    for (int s = EL_ASP_WH; s <= EL_FC_B; ++s) SDK_REQUIRE(d->off[tbs + s] >= 0, "%s: tail weight slot %d missing", fn, s);
  }
  return 0;
}

int ecapa_forward_impl(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf, int B, int T, void* ws, size_t ws_bytes,
                       float* emb, float* calib, void* stream) {
  typedef sdk_conv_gemm_args G;
  SDK_REQUIRE(ctx && wblob && feats && ws && emb, "sdk_ecapa_forward: null argument");
  if (int rc = check_desc(d)) return rc;
  if (int rc = check_forward_args("sdk_ecapa_forward", wblob, d, ldf, B, T, ws, ws_bytes, "sdk_ecapa_workspace_bytes", sdk_ecapa_workspace_bytes(d, B, T))) return rc;
  if (d->precision == 1) return ecapa_forward_hp(ctx, wblob, d, feats, ldf, B, T, ws, emb, stream);
  FwdWs w;
  fwd_carve({(char*)ws, 0}, d, B, T, &w);
  const Blob blob{(const char*)wblob, d->off};
  bool fuse_ctx = false, h_kb = false;
  if (int rc = ecapa_trunk(ctx, blob, d, feats, ldf, B, T, w, calib, stream, true, &fuse_ctx, &h_kb)) return rc;
  const int M = B * T, Cm = d->mfa_channels, A = d->attn_channels;
  const bool f16 = d->precision == 2;
  const uint32_t fmt = f16 ? SDK_GEMM_F16 : 0u;
  const int tb = EL_TAIL_BASE(d->n_blocks);
  if (fuse_ctx) {
    if (int rc = sdk_colstats_finish(ctx, w.stats, M, Cm, T, 2, w.ctx, stream)) return rc;
  } else {
    if (int rc = asp_stats_impl(ctx, w.H, Cm, B, T, Cm, w.ctx, stream, f16)) return rc;
  }
  if (int rc = sdk_rows_fc(ctx, w.ctx, 2 * Cm, nullptr, nullptr, blob.p32(tb + EL_ASP_WMS_T), blob.p32(tb + EL_ASP_B), w.ubias, A, B, 2 * Cm, A, 0, stream)) return rc;
  if (int rc = asp_hidden_gemm<G>(ctx, blob, tb, w.H, Cm, w.AH, A, w.ubias, A, M, Cm, A, T, (h_kb ? SDK_GEMM_A_KBLOCKED : 0) | fmt, stream)) return rc;
  if (A == 128 && T <= sdk_asp_fused_max_frames()) {
    // logits GEMM + softmax pooling fused: no [M, Cm] fp32 logits round trip through HBM
    if (int rc = asp_fused_launch(ctx, w.AH, A, blob.p16(tb + EL_ASP_W2), blob.p16(tb + EL_ASP_W2PACK), blob.p32(tb + EL_ASP_B2), w.H, Cm, B, T, Cm, A, w.pooled, stream, h_kb, f16)) return rc;
  } else {
    if (int rc = asp_logits_gemm<G>(ctx, blob, tb, w.AH, A, w.logits, M, Cm, A, T, fmt, stream)) return rc;
    if (int rc = asp_pool_impl(ctx, w.logits, Cm, w.H, Cm, B, T, Cm, w.pooled, stream, f16)) return rc;
  }
  return sdk_rows_fc(ctx, w.pooled, 2 * Cm, blob.p32(tb + EL_ASPBN_SCALE), blob.p32(tb + EL_ASPBN_SHIFT), blob.p32(tb + EL_FC_WT), blob.p32(tb + EL_FC_B), emb,
                     d->embed_dim, B, 2 * Cm, d->embed_dim, 0, stream);
}

// ---- ECAPA forward with S masked poolings per chunk (diarize.py: one per local speaker of a 10-s chunk; the rule is in sdk_hip.h and
// csrc/asp_masked.hip).  The trunk runs once per chunk with h row-major; the mask enters at the pooling only: one masked statistics sweep for all
// B S rows, the context bias per row, then per slot the attention-hidden GEMM with that slot's bias rows (ubias row b S + s: ldub = S A), the
// logits GEMM into ONE reused fp32 buffer and the masked softmax pooling; asp_bn + fc over the B S rows; invalid rows zeroed.
struct MaskedWs {
  FwdWs f;
  float *ctx, *ubias, *pooled;
  int32_t* ok;                       // [B S]: valid != 0 and v1 > 0, written by the statistics sweep: the rows that are not zeros
};
size_t masked_carve(WsCarver c, const sdk_ecapa_desc* d, int B, int T, int S, MaskedWs* w) {
  c.off = fwd_carve(c, d, B, T, &w->f, true);
  const size_t R = (size_t)B * S, Cm = d->mfa_channels, A = d->attn_channels;
  w->ctx = c.take<float>(R * 2 * Cm);
  w->ubias = c.take<float>(R * A);
  w->pooled = c.take<float>(R * 2 * Cm);
  w->ok = c.take<int32_t>(R);
  return c.bytes();
}

}  // namespace

extern "C" size_t sdk_ecapa_workspace_bytes(const sdk_ecapa_desc* d, int B, int T) {
  if (!d || B <= 0 || T <= 0 || (int64_t)B * T >= (1ll << 31)) {
    sdk_set_error("sdk_ecapa_workspace_bytes: d=%p B=%d T=%d (a descriptor, B and T at least 1, B*T below 2^31)", (const void*)d, B, T);
    return 0;
  }
  FwdWs w;
  FwdWsHp whp;
  return d->precision == 1 ? fwd_carve_hp({}, d, B, T, &whp) : fwd_carve({}, d, B, T, &w);
}

extern "C" size_t sdk_ecapa_calib_floats(const sdk_ecapa_desc* d, int B) {
  if (!d || B <= 0) return 0;
  return calib_offset(d, B, d->n_blocks, 2);
}

extern "C" int sdk_ecapa_forward(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf,
                                 int B, int T, void* ws, size_t ws_bytes, float* emb, void* stream) {
  return ecapa_forward_impl(ctx, wblob, d, feats, ldf, B, T, ws, ws_bytes, emb, nullptr, stream);
}

extern "C" int sdk_ecapa_forward_calib(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf,
                                       int B, int T, void* ws, size_t ws_bytes, float* emb, float* calib, void* stream) {
  SDK_REQUIRE(calib && d && d->precision != 1, "sdk_ecapa_forward_calib: calib is null or the blob is a precise-mode blob (calibration serves the single-plane modes 0 and 2)");
  return ecapa_forward_impl(ctx, wblob, d, feats, ldf, B, T, ws, ws_bytes, emb, calib, stream);
}

extern "C" size_t sdk_ecapa_masked_workspace_bytes(const sdk_ecapa_desc* d, int B, int T, int S) {
  if (!d || B <= 0 || T <= 0 || S < 1 || S > 8 || (int64_t)B * T >= (1ll << 31) || d->precision == 1) {
    sdk_set_error("sdk_ecapa_masked_workspace_bytes: d=%p B=%d T=%d S=%d precision=%d (a descriptor of precision 0 or 2, B and T at least 1, B*T below 2^31, S 1 .. 8)",
                  (const void*)d, B, T, S, d ? d->precision : -1);
    return 0;
  }
  MaskedWs w;
  return masked_carve({}, d, B, T, S, &w);
}

extern "C" int sdk_ecapa_forward_masked(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf, int B, int T, int S,
                                        const float* wgt, const int32_t* valid, void* ws, size_t ws_bytes, float* emb, void* stream) {
  typedef sdk_conv_gemm_args G;
  SDK_REQUIRE(ctx && wblob && feats && ws && emb, "sdk_ecapa_forward_masked: null pointer (ctx=%p wblob=%p feats=%p ws=%p emb=%p)", (void*)ctx, wblob,
              (const void*)feats, ws, (void*)emb);
  SDK_REQUIRE(wgt && valid, "sdk_ecapa_forward_masked: null pointer (w=%p valid=%p)", (const void*)wgt, (const void*)valid);
  if (int rc = check_desc(d)) return rc;
  SDK_REQUIRE(d->precision != 1, "sdk_ecapa_forward_masked: precision 1 (the precise mode's fp16 hi+lo planes) is not built for the masked pooling; use a blob of precision 0 (bf16) or 2 (fp16)");
  SDK_REQUIRE(S >= 1 && S <= 8, "sdk_ecapa_forward_masked: S=%d weight rows per chunk (served: 1 .. 8)", S);
  SDK_REQUIRE((int64_t)B * S < (1ll << 31), "sdk_ecapa_forward_masked: B*S overflows int32; split the batch");
  if (int rc = check_forward_args("sdk_ecapa_forward_masked", wblob, d, ldf, B, T, ws, ws_bytes, "sdk_ecapa_masked_workspace_bytes", sdk_ecapa_masked_workspace_bytes(d, B, T, S))) return rc;

  MaskedWs w;
  masked_carve({(char*)ws, 0}, d, B, T, S, &w);
  const Blob blob{(const char*)wblob, d->off};   // (every tail slot read below is one check_forward_args has required)
  bool fuse_ctx = false, h_kb = false;
  if (int rc = ecapa_trunk(ctx, blob, d, feats, ldf, B, T, w.f, nullptr, stream, false, &fuse_ctx, &h_kb)) return rc;
  const int M = B * T, Cm = d->mfa_channels, A = d->attn_channels, R = B * S, tb = EL_TAIL_BASE(d->n_blocks);
  const bool f16 = d->precision == 2;
  const uint32_t fmt = f16 ? SDK_GEMM_F16 : 0u;
  if (int rc = asp_stats_masked_impl(ctx, w.f.H, Cm, B, T, Cm, S, wgt, valid, w.ctx, stream, f16, w.ok)) return rc;
  if (int rc = sdk_rows_fc(ctx, w.ctx, 2 * Cm, nullptr, nullptr, blob.p32(tb + EL_ASP_WMS_T), blob.p32(tb + EL_ASP_B), w.ubias, A, R, 2 * Cm, A, 0, stream)) return rc;
  for (int s = 0; s < S; ++s) {
    if (int rc = asp_hidden_gemm<G>(ctx, blob, tb, w.f.H, Cm, w.f.AH, A, w.ubias + (int64_t)s * A, (int64_t)S * A, M, Cm, A, T, fmt, stream)) return rc;
    if (int rc = asp_logits_gemm<G>(ctx, blob, tb, w.f.AH, A, w.f.logits, M, Cm, A, T, fmt, stream)) return rc;
    if (int rc = asp_pool_masked_impl(ctx, w.f.logits, Cm, w.f.H, Cm, B, T, Cm, S, s, wgt, w.ok, w.pooled, stream, f16)) return rc;
  }
  if (int rc = sdk_rows_fc(ctx, w.pooled, 2 * Cm, blob.p32(tb + EL_ASPBN_SCALE), blob.p32(tb + EL_ASPBN_SHIFT), blob.p32(tb + EL_FC_WT), blob.p32(tb + EL_FC_B), emb,
                           d->embed_dim, R, 2 * Cm, d->embed_dim, 0, stream)) return rc;
  return resnet_zero_invalid_impl(ctx, emb, R, d->embed_dim, w.ok, stream);      // (the row-zeroing kernel of the ResNet34 family's masked forward)
}
