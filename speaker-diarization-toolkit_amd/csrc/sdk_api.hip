// libsdk_hip.so: context / error plumbing and the ECAPA-TDNN forward schedule (one C call per
// batch of segments; every step is an asynchronous launch on the caller's stream, so the whole
// forward can be captured in a hipGraph by the host).
#include <stdarg.h>
#include <string.h>

#include "common.hpp"
#include "ecapa_layout.h"
#include "hp.hpp"

static thread_local char g_err[512] = "";

void sdk_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* sdk_last_error(void) { return g_err; }
extern "C" int sdk_abi_version(void) { return SDK_ABI_VERSION; }

extern "C" int sdk_init(int device, sdk_ctx** out) {
  SDK_REQUIRE(out, "sdk_init: out is null");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    sdk_set_error("sdk_init: no HIP device available (%s); this library has no CPU fallback",
                  e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    return 1;
  }
  SDK_REQUIRE(device >= 0 && device < n, "sdk_init: device %d out of range (0..%d)", device, n - 1);
  sdk_ctx* c = new sdk_ctx();
  c->device = device;
  if (hipGetDeviceProperties(&c->prop, device) != hipSuccess) {
    delete c;
    sdk_set_error("sdk_init: hipGetDeviceProperties failed");
    return 1;
  }
  if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
    sdk_set_error("sdk_init: device %d is %s; libsdk_hip.so carries gfx950 (MI355X) code objects only", device,
                  c->prop.gcnArchName);
    delete c;
    return 1;
  }
  c->num_cu = c->prop.multiProcessorCount;
  SDK_HIP_OK(hipSetDevice(device));
  *out = c;
  return 0;
}

int sdk_lds_optin(sdk_ctx* ctx, const void* func, int bytes) {
  for (const void* f : ctx->lds_optin)
    if (f == func) return 0;
  SDK_HIP_OK(hipSetDevice(ctx->device));
  SDK_HIP_OK(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  ctx->lds_optin.push_back(func);
  return 0;
}

// ---- device memory for hosts that bring no allocator of their own (a C / C++ host, or the torch-free Python path lite.py) -----------
extern "C" int sdk_device_malloc(sdk_ctx* ctx, size_t bytes, void** out) {
  SDK_REQUIRE(ctx && out, "sdk_device_malloc: null argument");
  *out = nullptr;
  SDK_HIP_OK(hipSetDevice(ctx->device));
  SDK_HIP_OK(hipMalloc(out, bytes ? bytes : 1));
  return 0;
}
extern "C" int sdk_device_free(sdk_ctx* ctx, void* p) {
  SDK_REQUIRE(ctx, "sdk_device_free: null context");
  if (p) SDK_HIP_OK(hipFree(p));
  return 0;
}
// kind 1 = host -> device, 2 = device -> host, 3 = device -> device; ordered on `stream`, and the call returns when the copy is complete
extern "C" int sdk_memcpy(sdk_ctx* ctx, void* dst, const void* src, size_t bytes, int kind, void* stream) {
  SDK_REQUIRE(ctx && (bytes == 0 || (dst && src)), "sdk_memcpy: null argument");
  SDK_REQUIRE(kind >= 1 && kind <= 3, "sdk_memcpy: kind=%d (1 = host to device, 2 = device to host, 3 = device to device)", kind);
  if (!bytes) return 0;
  const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  SDK_HIP_OK(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
  SDK_HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
extern "C" int sdk_stream_synchronize(sdk_ctx* ctx, void* stream) {
  SDK_REQUIRE(ctx, "sdk_stream_synchronize: null context");
  SDK_HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

extern "C" int sdk_shutdown(sdk_ctx* ctx) {
  delete ctx;
  return 0;
}

extern "C" int sdk_get_device_info(sdk_ctx* ctx, sdk_device_info* out) {
  SDK_REQUIRE(ctx && out, "sdk_get_device_info: null argument");
  memset(out, 0, sizeof(*out));
  out->device = ctx->device;
  out->compute_units = ctx->prop.multiProcessorCount;
  out->clock_khz = ctx->prop.clockRate;
  out->wavefront_size = ctx->prop.warpSize;
  out->hbm_bytes = ctx->prop.totalGlobalMem;
  strncpy(out->name, ctx->prop.name, sizeof(out->name) - 1);
  strncpy(out->arch, ctx->prop.gcnArchName, sizeof(out->arch) - 1);
  return 0;
}

extern "C" int sdk_set_option(sdk_ctx* ctx, const char* name, int value) {
  SDK_REQUIRE(ctx && name, "sdk_set_option: null argument");
  if (strcmp(name, "res2net_chain_fusion") == 0) { ctx->no_chain_fusion = value == 0; return 0; }
  if (strcmp(name, "res2net_packed_weights") == 0) { ctx->no_chain_packed = value == 0; return 0; }
  if (strcmp(name, "res2net_two_per_cu") == 0) { ctx->no_chain_two_per_cu = value == 0; return 0; }
  if (strcmp(name, "asp_packed_weights") == 0) { ctx->no_asp_packed = value == 0; return 0; }
  if (strcmp(name, "asp_per_segment") == 0) { ctx->no_asp_seg = value == 0; return 0; }
  if (strcmp(name, "h_kblocked") == 0) { ctx->no_h_kblocked = value == 0; return 0; }
  if (strcmp(name, "precision") == 0) {
    SDK_REQUIRE(value >= 0 && value <= 2, "sdk_set_option: precision must be 0 (bf16 operands), 1 (fp16 hi+lo planes) or 2 (one fp16 plane), got %d", value);
    ctx->precision = value;
    return 0;
  }
  if (strcmp(name, "gemm_variant") == 0) return sdk_set_gemm_variant(value);
  if (strcmp(name, "affinity_fast_path") == 0) { ctx->aff_fast = value; return 0; }
  if (strcmp(name, "affinity_variant") == 0) { ctx->aff_variant = value; return 0; }
  if (strcmp(name, "affinity_boundary_penalty") == 0) { ctx->aff_boundary_pen = value < 0 ? 0 : value; return 0; }
  if (strcmp(name, "matvec_variant") == 0) { ctx->matvec_variant = value; return 0; }
  if (strcmp(name, "hp_gemm_variant") == 0) { ctx->hp_gemm_variant = value; return 0; }
  if (strcmp(name, "affinity_whole_groups") == 0) return 0;      // (round-3 knob, measured behind and removed in round 5: accepted and ignored)
  if (strcmp(name, "chol_pivot_rtol_ppb") == 0) { ctx->chol_pivot_rtol_ppb = value < 0 ? 0 : value; return 0; }
  if (strcmp(name, "chol_shift_ppb") == 0) { ctx->chol_shift_ppb = value < 0 ? 0 : value; return 0; }
  if (strcmp(name, "ahc_distances_only") == 0) { ctx->ahc_distances_only = value != 0; return 0; }
  if (strcmp(name, "snorm_scores_only") == 0) { ctx->snorm_scores_only = value != 0; return 0; }
  if (strcmp(name, "trials_no_hist") == 0) { ctx->trials_no_hist = value != 0; return 0; }
  sdk_set_error("sdk_set_option: unknown option '%s'", name);
  return 2;
}

extern "C" int sdk_debug_set_ptr(sdk_ctx* ctx, const char* name, void* p) {
  SDK_REQUIRE(ctx && name, "sdk_debug_set_ptr: null argument");
  if (strcmp(name, "stamps") == 0) { ctx->dbg_ptr = p; return 0; }
  if (strcmp(name, "gemm_clock") == 0) { ctx->gemm_clk_ptr = p; return 0; }
  if (strcmp(name, "gemm_stamps") == 0) { ctx->gemm_stamps_ptr = p; return 0; }
  sdk_set_error("sdk_debug_set_ptr: unknown name '%s'", name);
  return 2;
}

extern "C" int sdk_profile_begin(sdk_ctx* ctx) {
  SDK_REQUIRE(ctx, "sdk_profile_begin: null ctx");
  for (auto& r : ctx->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  ctx->prof.clear();
  ctx->prof_on = true;
  return 0;
}

extern "C" int sdk_profile_end(sdk_ctx* ctx, sdk_profile_report* out) {
  SDK_REQUIRE(ctx && out, "sdk_profile_end: null argument");
  ctx->prof_on = false;
  memset(out, 0, sizeof(*out));
  SDK_HIP_OK(hipDeviceSynchronize());
  for (auto& r : ctx->prof) {
    float ms = 0.f;
    SDK_HIP_OK(hipEventElapsedTime(&ms, r.a, r.b));
    if (r.family >= 0 && r.family < SDK_K_COUNT) {
      out->launches[r.family] += 1;
      out->ms[r.family] += ms;
      out->flops[r.family] += r.flops;
      out->bytes[r.family] += r.bytes;
    }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  ctx->prof.clear();
  return 0;
}

// ------------------------------------------------------------------------------ ECAPA forward
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
// attention logits in fp32 through HBM): this mode buys accuracy, the default mode is the fast one.
int ecapa_forward_hp(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf, int B, int T, void* ws,
                     float* emb, void* stream) {
  FwdWsHp w;
  fwd_carve_hp({(char*)ws, 0}, d, B, T, &w);
  const char* wb = (const char*)wblob;
  auto P16 = [&](int slot) -> const uint16_t* { return d->off[slot] < 0 ? nullptr : (const uint16_t*)(wb + d->off[slot]); };
  auto P32 = [&](int slot) -> const float* { return d->off[slot] < 0 ? nullptr : (const float*)(wb + d->off[slot]); };
  const int M = B * T, C = d->channels, Cm = d->mfa_channels, S = d->sub_channels, A = d->attn_channels;
  const int flo = ldf >> 1;
  SDK_REQUIRE(ldf % 16 == 0 && flo >= d->n_mels_padded, "sdk_ecapa_forward: precise mode takes feature planes, ldf=%d must be >= 2 x %d", ldf, d->n_mels_padded);

  auto tdnn = [&](const uint16_t* Ain, int64_t lda, int64_t a_lo, int Cin, int taps, int dil, int slot, int N, uint16_t* Cout, int64_t ldc, int64_t c_lo,
                  const uint16_t* X2, int64_t ldx2, int64_t x2_lo, uint16_t* Sout, int64_t lds, int64_t s_lo) -> int {
    sdk_conv_gemm_hp_args g;
    memset(&g, 0, sizeof(g));
    g.A = Ain; g.lda = lda; g.a_lo = a_lo; g.W = P16(slot + EL_W); g.C = Cout; g.ldc = ldc; g.c_lo = c_lo;
    g.bias = P32(slot + EL_B); g.scale = P32(slot + EL_SCALE); g.shift = P32(slot + EL_SHIFT);
    g.X2 = X2; g.ldx2 = ldx2; g.x2_lo = x2_lo; g.S = Sout; g.lds = lds; g.s_lo = s_lo;
    g.M = M; g.N = N; g.Cin = Cin; g.taps = taps; g.dil = dil; g.T = T; g.flags = SDK_GEMM_RELU;
    SDK_REQUIRE(g.W && g.bias && g.scale && g.shift, "sdk_ecapa_forward: weight slot %d missing", slot);
    return sdk_conv_gemm_hp(ctx, &g, stream);
  };
  hipStream_t st = (hipStream_t)stream;

  if (int rc = tdnn(feats, ldf, flo, d->n_mels_padded, d->kernel0, 1, EL_BLK0, C, w.X0, 2 * C, C, nullptr, 0, 0, nullptr, 0, 0)) return rc;
  const uint16_t* xin = w.X0;
  int64_t ldx = 2 * C, xlo = C;
  for (int i = 1; i <= d->n_blocks; ++i) {
    const int base = EL_BLOCK_BASE(i), dil = d->dilation[i - 1];
    if (int rc = tdnn(xin, ldx, xlo, C, 1, 1, base + EL_TDNN1, C, w.U, 2 * C, C, nullptr, 0, 0, nullptr, 0, 0)) return rc;
    {   // Res2Net chunk 0 passes through: both planes
      ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 2.0 * M * S * 4);
      SDK_HIP_OK(hipMemcpy2DAsync(w.R, (size_t)C * 4, w.U, (size_t)C * 4, (size_t)S * 2, (size_t)M, hipMemcpyDeviceToDevice, st));
      SDK_HIP_OK(hipMemcpy2DAsync(w.R + C, (size_t)C * 4, w.U + C, (size_t)C * 4, (size_t)S * 2, (size_t)M, hipMemcpyDeviceToDevice, st));
    }
    for (int j = 0; j < d->scale - 1; ++j) {
      const uint16_t* Ain = j == 0 ? w.U + S : ((j & 1) ? w.Sa : w.Sb);
      const int64_t lda = j == 0 ? 2 * C : 2 * S, alo = j == 0 ? C : S;
      const bool more = j + 1 < d->scale - 1;
      uint16_t* Sout = more ? ((j & 1) ? w.Sb : w.Sa) : nullptr;
      const uint16_t* X2 = more ? w.U + (int64_t)S * (j + 2) : nullptr;
      if (int rc = tdnn(Ain, lda, alo, S, 3, dil, base + EL_RES2NET(j), S, w.R + (int64_t)S * (j + 1), 2 * C, C, X2, 2 * C, C, Sout, 2 * S, S)) return rc;
    }
    if (int rc = tdnn(w.R, 2 * C, C, C, 1, 1, base + EL_TDNN2, C, w.Z, 2 * C, C, nullptr, 0, 0, nullptr, 0, 0)) return rc;
    // squeeze-excitation: mean sweep, two per-utterance FCs (fp32 matrix pipe), apply sweep
    if (int rc = hp_seg_mean(ctx, w.Z, 2 * C, C, B, T, C, w.mean, stream)) return rc;
    if (int rc = sdk_rows_fc(ctx, w.mean, C, nullptr, nullptr, P32(base + EL_SE_W1T), P32(base + EL_SE_B1), w.hid, d->se_channels, B, C, d->se_channels, 1, stream)) return rc;
    if (int rc = sdk_rows_fc(ctx, w.hid, d->se_channels, nullptr, nullptr, P32(base + EL_SE_W2T), P32(base + EL_SE_B2), w.gate, C, B, d->se_channels, C, 2, stream)) return rc;
    uint16_t* slab = w.CAT + (int64_t)C * (i - 1);
    if (int rc = hp_se_apply(ctx, w.Z, 2 * C, C, xin, ldx, xlo, w.gate, slab, 2 * Cm, Cm, B, T, C, stream)) return rc;
    xin = slab;
    ldx = 2 * Cm;
    xlo = Cm;
  }
  const int tb = EL_TAIL_BASE(d->n_blocks);
  if (int rc = tdnn(w.CAT, 2 * Cm, Cm, Cm, 1, 1, tb + EL_MFA, Cm, w.H, 2 * Cm, Cm, nullptr, 0, 0, nullptr, 0, 0)) return rc;
  if (int rc = hp_asp_stats(ctx, w.H, 2 * Cm, Cm, B, T, Cm, w.ctx, stream)) return rc;
  if (int rc = sdk_rows_fc(ctx, w.ctx, 2 * Cm, nullptr, nullptr, P32(tb + EL_ASP_WMS_T), P32(tb + EL_ASP_B), w.ubias, A, B, 2 * Cm, A, 0, stream)) return rc;
  {
    sdk_conv_gemm_hp_args g;
    memset(&g, 0, sizeof(g));
    g.A = w.H; g.lda = 2 * Cm; g.a_lo = Cm; g.W = P16(tb + EL_ASP_WH); g.C = w.AH; g.ldc = 2 * A; g.c_lo = A;
    g.ubias = w.ubias; g.ldub = A; g.scale = P32(tb + EL_ASP_SCALE); g.shift = P32(tb + EL_ASP_SHIFT);
    g.M = M; g.N = A; g.Cin = Cm; g.taps = 1; g.dil = 1; g.T = T; g.flags = SDK_GEMM_RELU | SDK_GEMM_TANH;
    if (int rc = sdk_conv_gemm_hp(ctx, &g, stream)) return rc;
    memset(&g, 0, sizeof(g));
    g.A = w.AH; g.lda = 2 * A; g.a_lo = A; g.W = P16(tb + EL_ASP_W2); g.C32 = w.logits; g.ldc32 = Cm; g.bias = P32(tb + EL_ASP_B2);
    g.M = M; g.N = Cm; g.Cin = A; g.taps = 1; g.dil = 1; g.T = T; g.flags = 0;
    if (int rc = sdk_conv_gemm_hp(ctx, &g, stream)) return rc;
  }
  if (int rc = hp_asp_pool(ctx, w.logits, Cm, w.H, 2 * Cm, Cm, B, T, Cm, w.pooled, stream)) return rc;
  return sdk_rows_fc(ctx, w.pooled, 2 * Cm, P32(tb + EL_ASPBN_SCALE), P32(tb + EL_ASPBN_SHIFT), P32(tb + EL_FC_WT), P32(tb + EL_FC_B), emb,
                     d->embed_dim, B, 2 * Cm, d->embed_dim, 0, stream);
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

// Calibration slots (sdk_ecapa_forward_calib): per-segment mean | std (sdk_asp_stats layout [B, 2 C_l]) of the INPUT of every bf16 GEMM layer whose
// weight rounding the host corrects in the bias (weights_pack.bias_corrections): per block tdnn1, the Res2Net convs, tdnn2; then MFA, ASP hidden.
static size_t calib_offset(const sdk_ecapa_desc* d, int B, int block, int layer) {   // block < n_blocks: layer 0 = tdnn1, 1..scale-1 = Res2Net conv
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

extern "C" size_t sdk_ecapa_calib_floats(const sdk_ecapa_desc* d, int B) {
  if (!d || B <= 0) return 0;
  return calib_offset(d, B, d->n_blocks, 2);
}

static int ecapa_forward_impl(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf,
                              int B, int T, void* ws, size_t ws_bytes, float* emb, float* calib, void* stream);

extern "C" int sdk_ecapa_forward(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf,
                                 int B, int T, void* ws, size_t ws_bytes, float* emb, void* stream) {
  return ecapa_forward_impl(ctx, wblob, d, feats, ldf, B, T, ws, ws_bytes, emb, nullptr, stream);
}

extern "C" int sdk_ecapa_forward_calib(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf,
                                       int B, int T, void* ws, size_t ws_bytes, float* emb, float* calib, void* stream) {
  SDK_REQUIRE(calib && d && d->precision != 1, "sdk_ecapa_forward_calib: calib is null or the blob is a precise-mode blob (calibration serves the single-plane modes 0 and 2)");
  return ecapa_forward_impl(ctx, wblob, d, feats, ldf, B, T, ws, ws_bytes, emb, calib, stream);
}

// The trunk shared by sdk_ecapa_forward and sdk_ecapa_forward_masked: blk0, the SE-Res2Net blocks and MFA, feats -> h [M, Cm] in w.H (K-blocked
// where *h_kb), with the fused column statistics of h in w.stats where *fuse_ctx.  One function, so that the masked forward's h is the
// unmasked forward's bit for bit at the same (B, T): the same launches with the same arguments.  allow_kblocked = false only changes where
// the MFA epilogue stores a value, not the value - on the default GEMM dispatch.  ONE EXCEPTION, reachable through the A/B knob alone: with
// "gemm_variant" 1 (SDK_GEMM_VARIANT=1: every GEMM on the 128^2 kernel) a K-blocked output still forces the 256^2 kernel (sdk_conv_gemm), so
// where the unmasked forward writes h K-blocked (96 < T <= 208 by default) its MFA runs another kernel than the masked forward's and h agrees
// to fp32 summation order only.  At diarization's T = 1001 neither forward writes h K-blocked, whatever the knob.
static int ecapa_trunk(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf, int B, int T, const FwdWs& w,
                       float* calib, void* stream, bool allow_kblocked, bool* fuse_ctx_out, bool* h_kb_out) {
  const char* wb = (const char*)wblob;
  auto P16 = [&](int slot) -> const uint16_t* { return d->off[slot] < 0 ? nullptr : (const uint16_t*)(wb + d->off[slot]); };
  auto P32 = [&](int slot) -> const float* { return d->off[slot] < 0 ? nullptr : (const float*)(wb + d->off[slot]); };
  const int M = B * T, C = d->channels, Cm = d->mfa_channels, S = d->sub_channels, A = d->attn_channels;
  hipStream_t st = (hipStream_t)stream;
  // precision 2 (round 5): the same schedule with every 2-byte tensor - features, weights, activations - in fp16 instead of bf16 (11 significand
  // bits: 7 x closer to the fp32 model at one MFMA per product, profiles/r05_fp16_decision.txt); every stage takes the
  // format per call: the GEMMs from their flag, the sweeps and the two fused launches from an argument of their internal entry
  const bool f16 = d->precision == 2;
  const uint32_t fmt = f16 ? SDK_GEMM_F16 : 0u;

  auto tdnn = [&](const uint16_t* Ain, int64_t lda, int Cin, int taps, int dil, int slot, int N, uint16_t* Cout, int64_t ldc,
                  const uint16_t* X2, int64_t ldx2, uint16_t* Sout, int64_t lds, int stats_mode = 0, uint32_t layout = 0) -> int {
    sdk_conv_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = Ain; g.lda = lda; g.W = P16(slot + EL_W); g.C = Cout; g.ldc = ldc;
    g.bias = P32(slot + EL_B); g.scale = P32(slot + EL_SCALE); g.shift = P32(slot + EL_SHIFT);
    g.X2 = X2; g.ldx2 = ldx2; g.S = Sout; g.lds = lds;
    g.M = M; g.N = N; g.Cin = Cin; g.taps = taps; g.dil = dil; g.T = T; g.flags = SDK_GEMM_RELU | layout | fmt;
    g.stats_mode = stats_mode; g.stats_part = stats_mode ? w.stats : nullptr;
    SDK_REQUIRE(g.W && g.bias && g.scale && g.shift, "sdk_ecapa_forward: weight slot %d missing", slot);
    return sdk_conv_gemm(ctx, &g, stream);
  };

  // blk0: k5 conv over the mel channels; with a packed weight slot the five taps share K (5 x 80 -> 448: 7 K-steps instead of 10)
  if (d->blk0_tap_pack > 0) {
    sdk_conv_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = feats; g.lda = ldf; g.W = P16(EL_BLK0 + EL_W); g.C = w.X0; g.ldc = C;
    g.bias = P32(EL_BLK0 + EL_B); g.scale = P32(EL_BLK0 + EL_SCALE); g.shift = P32(EL_BLK0 + EL_SHIFT);
    g.M = M; g.N = C; g.Cin = d->blk0_tap_pack; g.taps = d->kernel0; g.dil = 1; g.T = T; g.flags = SDK_GEMM_RELU | fmt; g.tap_pack = d->blk0_tap_pack;
    SDK_REQUIRE(g.W && g.bias && g.scale && g.shift && d->blk0_tap_pack <= ldf, "sdk_ecapa_forward: blk0 weight slots missing or tap_pack > ldf");
    if (int rc = sdk_conv_gemm(ctx, &g, stream)) return rc;
  } else if (int rc = tdnn(feats, ldf, d->n_mels_padded, d->kernel0, 1, EL_BLK0, C, w.X0, C, nullptr, 0, nullptr, 0)) return rc;

  const uint16_t* xin = w.X0;
  int64_t ldx = C;
  for (int i = 1; i <= d->n_blocks; ++i) {
    const int base = EL_BLOCK_BASE(i), dil = d->dilation[i - 1];
    if (calib)
      if (int rc = asp_stats_impl(ctx, xin, ldx, B, T, C, calib + calib_offset(d, B, i - 1, 0), stream, f16)) return rc;
    if (int rc = tdnn(xin, ldx, C, 1, 1, base + EL_TDNN1, C, w.U, C, nullptr, 0, nullptr, 0)) return rc;
    // Res2Net: chunk 0 passes through, chunk c>=1 = TDNN(chunk c + y_{c-1})
    const uint16_t* r2out = w.R;
    if (S == 128 && d->scale - 1 <= 7 && T <= sdk_res2net_chain_max_frames() && !ctx->no_chain_fusion && !calib) {
      // the seven dependent convolutions in ONE launch, the running tile resident in LDS per segment.  The chain runs
      // IN PLACE on the tdnn1 output: a workgroup has read u_c (into LDS / registers) before it writes y_c over it, and
      // segments do not overlap - so chunk 0 needs no copy
      const uint16_t* Wp[7]; const uint16_t* Wk[7]; const float* bp[7]; const float* sp[7]; const float* tp[7];
      for (int j = 0; j < d->scale - 1; ++j) {
        const int slot = base + EL_RES2NET(j);
        Wp[j] = P16(slot + EL_W); bp[j] = P32(slot + EL_B); sp[j] = P32(slot + EL_SCALE); tp[j] = P32(slot + EL_SHIFT);
        Wk[j] = (i <= 4 && d->off[EL_CHAINPACK(i, j)] >= 0) ? P16(EL_CHAINPACK(i, j)) : nullptr;   // optional fragment-ordered copy
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
        if (calib)
          if (int rc = asp_stats_impl(ctx, Ain, lda, B, T, S, calib + calib_offset(d, B, i - 1, 1 + j), stream, f16)) return rc;
        if (int rc = tdnn(Ain, lda, S, 3, dil, base + EL_RES2NET(j), S, w.R + (int64_t)S * (j + 1), C, X2, C, Sout, S)) return rc;
      }
    }
    if (calib)
      if (int rc = asp_stats_impl(ctx, r2out, C, B, T, C, calib + calib_offset(d, B, i - 1, d->scale), stream, f16)) return rc;
    // the SE squeeze (per-segment channel means of z) comes out of the tdnn2 epilogue where the shape allows it
    const bool fuse_se = sdk_conv_gemm_stats_fusable(M, C, T) != 0;
    if (int rc = tdnn(r2out, C, C, 1, 1, base + EL_TDNN2, C, w.Z, C, nullptr, 0, nullptr, 0, fuse_se ? 1 : 0)) return rc;
    if (fuse_se)
      if (int rc = sdk_colstats_finish(ctx, w.stats, M, C, T, 1, w.mean, stream)) return rc;
    uint16_t* slab = w.CAT + (int64_t)C * (i - 1);
    if (int rc = se_gate_residual_impl(ctx, w.Z, C, xin, ldx, P32(base + EL_SE_W1T), P32(base + EL_SE_B1), P32(base + EL_SE_W2T),
                                       P32(base + EL_SE_B2), slab, Cm, B, T, C, d->se_channels, fuse_se ? w.mean : nullptr, w.se,
                                       sdk_se_workspace_bytes(B, C, d->se_channels), stream, f16)) return rc;
    xin = slab;
    ldx = Cm;
  }

  const int tb = EL_TAIL_BASE(d->n_blocks);
  // attentive statistics pooling with global context; the context (mean | std of h over frames) comes out of
  // the MFA epilogue where the shape allows it, else from a separate sweep of h
  const bool fuse_ctx = sdk_conv_gemm_stats_fusable(M, Cm, T) != 0;
  if (calib)
    if (int rc = asp_stats_impl(ctx, w.CAT, Cm, B, T, Cm, calib + calib_offset(d, B, d->n_blocks, 0), stream, f16)) return rc;
  // h [M, Cm] is the widest activation and is read twice, both times in 64- / 32-channel pieces of its 6-KB rows (the skinny attention-hidden GEMM,
  // the per-segment ASP slabs): where those two are its only readers it is written K-BLOCKED, [Cm / 64][M][64] (sdk_hip.h SDK_GEMM_C_KBLOCKED)
  const bool h_kb = allow_kblocked && !ctx->no_h_kblocked && !calib && fuse_ctx && A == 128 && sdk_asp_kblocked_ok(ctx, T, Cm) != 0;
  if (int rc = tdnn(w.CAT, Cm, Cm, 1, 1, tb + EL_MFA, Cm, w.H, Cm, nullptr, 0, nullptr, 0, fuse_ctx ? 2 : 0, h_kb ? SDK_GEMM_C_KBLOCKED : 0)) return rc;
  if (calib)
    if (int rc = asp_stats_impl(ctx, w.H, Cm, B, T, Cm, calib + calib_offset(d, B, d->n_blocks, 1), stream, f16)) return rc;
  *fuse_ctx_out = fuse_ctx;
  *h_kb_out = h_kb;
  return 0;
}

// The checks both forwards make after their null-pointer and descriptor checks, in sdk_ecapa_forward's order and words (fn: the entry point's name;
// need: its workspace size): batch, feature width, receptive halo, workspace, alignment, weight slots.
static int check_forward_args(const char* fn, const void* wblob, const sdk_ecapa_desc* d, int ldf, int B, int T, const void* ws, size_t ws_bytes, const char* sizer, size_t need) {
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

static int ecapa_forward_impl(sdk_ctx* ctx, const void* wblob, const sdk_ecapa_desc* d, const uint16_t* feats, int ldf,
                              int B, int T, void* ws, size_t ws_bytes, float* emb, float* calib, void* stream) {
  SDK_REQUIRE(ctx && wblob && feats && ws && emb, "sdk_ecapa_forward: null argument");
  if (int rc = check_desc(d)) return rc;
  if (int rc = check_forward_args("sdk_ecapa_forward", wblob, d, ldf, B, T, ws, ws_bytes, "sdk_ecapa_workspace_bytes", sdk_ecapa_workspace_bytes(d, B, T))) return rc;
  if (d->precision == 1) return ecapa_forward_hp(ctx, wblob, d, feats, ldf, B, T, ws, emb, stream);
  FwdWs w;
  fwd_carve({(char*)ws, 0}, d, B, T, &w);
  bool fuse_ctx = false, h_kb = false;
  if (int rc = ecapa_trunk(ctx, wblob, d, feats, ldf, B, T, w, calib, stream, true, &fuse_ctx, &h_kb)) return rc;
  const char* wb = (const char*)wblob;
  auto P16 = [&](int slot) -> const uint16_t* { return d->off[slot] < 0 ? nullptr : (const uint16_t*)(wb + d->off[slot]); };
  auto P32 = [&](int slot) -> const float* { return d->off[slot] < 0 ? nullptr : (const float*)(wb + d->off[slot]); };
  const int M = B * T, Cm = d->mfa_channels, A = d->attn_channels;
  const bool f16 = d->precision == 2;
  const uint32_t fmt = f16 ? SDK_GEMM_F16 : 0u;
  const int tb = EL_TAIL_BASE(d->n_blocks);
  if (fuse_ctx) {
    if (int rc = sdk_colstats_finish(ctx, w.stats, M, Cm, T, 2, w.ctx, stream)) return rc;
  } else {
    if (int rc = asp_stats_impl(ctx, w.H, Cm, B, T, Cm, w.ctx, stream, f16)) return rc;
  }
  if (int rc = sdk_rows_fc(ctx, w.ctx, 2 * Cm, nullptr, nullptr, P32(tb + EL_ASP_WMS_T), P32(tb + EL_ASP_B), w.ubias, A, B, 2 * Cm, A, 0, stream)) return rc;
  {
    sdk_conv_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = w.H; g.lda = Cm; g.W = P16(tb + EL_ASP_WH); g.C = w.AH; g.ldc = A;
    g.ubias = w.ubias; g.ldub = A; g.scale = P32(tb + EL_ASP_SCALE); g.shift = P32(tb + EL_ASP_SHIFT);
    g.M = M; g.N = A; g.Cin = Cm; g.taps = 1; g.dil = 1; g.T = T; g.flags = SDK_GEMM_RELU | SDK_GEMM_TANH | (h_kb ? SDK_GEMM_A_KBLOCKED : 0) | fmt;
    if (int rc = sdk_conv_gemm(ctx, &g, stream)) return rc;
    if (A == 128 && T <= sdk_asp_fused_max_frames()) {
      // logits GEMM + softmax pooling fused: no [M, Cm] fp32 logits round trip through HBM
      if (int rc = asp_fused_launch(ctx, w.AH, A, P16(tb + EL_ASP_W2), P16(tb + EL_ASP_W2PACK), P32(tb + EL_ASP_B2), w.H, Cm, B, T, Cm, A, w.pooled, stream, h_kb, f16)) return rc;
    } else {
      memset(&g, 0, sizeof(g));
      g.A = w.AH; g.lda = A; g.W = P16(tb + EL_ASP_W2); g.C32 = w.logits; g.ldc32 = Cm; g.bias = P32(tb + EL_ASP_B2);
      g.M = M; g.N = Cm; g.Cin = A; g.taps = 1; g.dil = 1; g.T = T; g.flags = fmt;
      if (int rc = sdk_conv_gemm(ctx, &g, stream)) return rc;
      if (int rc = asp_pool_impl(ctx, w.logits, Cm, w.H, Cm, B, T, Cm, w.pooled, stream, f16)) return rc;
    }
  }
  return sdk_rows_fc(ctx, w.pooled, 2 * Cm, P32(tb + EL_ASPBN_SCALE), P32(tb + EL_ASPBN_SHIFT), P32(tb + EL_FC_WT),
                     P32(tb + EL_FC_B), emb, d->embed_dim, B, 2 * Cm, d->embed_dim, 0, stream);
}

// ------------------------------------------------------------------------------ ECAPA forward with S masked poolings per chunk
// (diarize.py: one per local speaker of a 10-s chunk; the rule is in sdk_hip.h and csrc/asp_masked.hip).  The trunk runs once per chunk
// with h row-major; the mask enters at the pooling only: one masked statistics sweep for all B S rows, the context bias per row, then per
// slot the attention-hidden GEMM with that slot's bias rows (ubias row b S + s: ldub = S A), the logits GEMM into ONE reused fp32 buffer and
// the masked softmax pooling; asp_bn + fc over the B S rows; invalid rows zeroed.
namespace {
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
  SDK_REQUIRE(ctx && wblob && feats && ws && emb, "sdk_ecapa_forward_masked: null pointer (ctx=%p wblob=%p feats=%p ws=%p emb=%p)", (void*)ctx, wblob,
              (const void*)feats, ws, (void*)emb);
  SDK_REQUIRE(wgt && valid, "sdk_ecapa_forward_masked: null pointer (w=%p valid=%p)", (const void*)wgt, (const void*)valid);
  if (int rc = check_desc(d)) return rc;
  SDK_REQUIRE(d->precision != 1, "sdk_ecapa_forward_masked: precision 1 (the precise mode's fp16 hi+lo planes) is not built for the masked pooling; use a blob of precision 0 (bf16) or 2 (fp16)");
  SDK_REQUIRE(S >= 1 && S <= 8, "sdk_ecapa_forward_masked: S=%d weight rows per chunk (served: 1 .. 8)", S);
  SDK_REQUIRE((int64_t)B * S < (1ll << 31), "sdk_ecapa_forward_masked: B*S overflows int32; split the batch");
  if (int rc = check_forward_args("sdk_ecapa_forward_masked", wblob, d, ldf, B, T, ws, ws_bytes, "sdk_ecapa_masked_workspace_bytes", sdk_ecapa_masked_workspace_bytes(d, B, T, S))) return rc;
  const int tb = EL_TAIL_BASE(d->n_blocks);

  MaskedWs w;
  masked_carve({(char*)ws, 0}, d, B, T, S, &w);
  bool fuse_ctx = false, h_kb = false;
  if (int rc = ecapa_trunk(ctx, wblob, d, feats, ldf, B, T, w.f, nullptr, stream, false, &fuse_ctx, &h_kb)) return rc;
  const char* wb = (const char*)wblob;
  auto P16 = [&](int slot) -> const uint16_t* { return (const uint16_t*)(wb + d->off[slot]); };
  auto P32 = [&](int slot) -> const float* { return (const float*)(wb + d->off[slot]); };
  const int M = B * T, Cm = d->mfa_channels, A = d->attn_channels, R = B * S;
  const bool f16 = d->precision == 2;
  const uint32_t fmt = f16 ? SDK_GEMM_F16 : 0u;
  if (int rc = asp_stats_masked_impl(ctx, w.f.H, Cm, B, T, Cm, S, wgt, valid, w.ctx, stream, f16, w.ok)) return rc;
  if (int rc = sdk_rows_fc(ctx, w.ctx, 2 * Cm, nullptr, nullptr, P32(tb + EL_ASP_WMS_T), P32(tb + EL_ASP_B), w.ubias, A, R, 2 * Cm, A, 0, stream)) return rc;
  for (int s = 0; s < S; ++s) {
    sdk_conv_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = w.f.H; g.lda = Cm; g.W = P16(tb + EL_ASP_WH); g.C = w.f.AH; g.ldc = A;
    g.ubias = w.ubias + (int64_t)s * A; g.ldub = (int64_t)S * A; g.scale = P32(tb + EL_ASP_SCALE); g.shift = P32(tb + EL_ASP_SHIFT);
    g.M = M; g.N = A; g.Cin = Cm; g.taps = 1; g.dil = 1; g.T = T; g.flags = SDK_GEMM_RELU | SDK_GEMM_TANH | fmt;
    if (int rc = sdk_conv_gemm(ctx, &g, stream)) return rc;
    memset(&g, 0, sizeof(g));
    g.A = w.f.AH; g.lda = A; g.W = P16(tb + EL_ASP_W2); g.C32 = w.f.logits; g.ldc32 = Cm; g.bias = P32(tb + EL_ASP_B2);
    g.M = M; g.N = Cm; g.Cin = A; g.taps = 1; g.dil = 1; g.T = T; g.flags = fmt;
    if (int rc = sdk_conv_gemm(ctx, &g, stream)) return rc;
    if (int rc = asp_pool_masked_impl(ctx, w.f.logits, Cm, w.f.H, Cm, B, T, Cm, S, s, wgt, w.ok, w.pooled, stream, f16)) return rc;
  }
  if (int rc = sdk_rows_fc(ctx, w.pooled, 2 * Cm, P32(tb + EL_ASPBN_SCALE), P32(tb + EL_ASPBN_SHIFT), P32(tb + EL_FC_WT), P32(tb + EL_FC_B), emb,
                           d->embed_dim, R, 2 * Cm, d->embed_dim, 0, stream)) return rc;
  return resnet_zero_invalid_impl(ctx, emb, R, d->embed_dim, w.ok, stream);      // (the row-zeroing kernel of the ResNet34 family's masked forward)
}

// ------------------------------------------------------------------------------ x-vector forward
// The plain TDNN embedding extractor (Snyder et al. 2018) composed from the same pieces: every frame layer is one sdk_conv_gemm
// (conv -> ReLU -> folded BN -> bf16), the pooled statistics and the embedding layer are fp32.
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
  SDK_REQUIRE_WS("sdk_xvector_forward", "sdk_xvector_workspace_bytes", ws, ws_bytes, sdk_xvector_workspace_bytes(d, B, T), 256);
  SDK_REQUIRE(((uintptr_t)wblob % 256) == 0, "sdk_xvector_forward: wblob=%p must be 256-byte aligned", wblob);
  XvWs w;
  xv_carve({(char*)ws, 0}, d, B, T, &w);
  uint16_t *const b0 = w.b0, *const b1 = w.b1;
  float* const stats = w.stats;
  const char* wb = (const char*)wblob;
  const uint16_t* in = feats;
  int64_t ldin = ldf;
  const int M = B * T;
  const int Cl = d->cout[d->n_frame_layers - 1];
  if (hp) {
    // precise mode (north_star's 1e-5): every frame layer on the fp16 hi+lo plane GEMM (three MFMAs per product, csrc/hp.hip), planes between the
    // layers, statistics pooling on the planes; the embedding layer is fp32 either way
    int64_t in_lo = ldf >> 1;
    for (int l = 0; l < d->n_frame_layers; ++l) {
      uint16_t* out = (l & 1) ? b1 : b0;
      sdk_conv_gemm_hp_args g;
      memset(&g, 0, sizeof(g));
      g.A = in; g.lda = ldin; g.a_lo = in_lo; g.W = (const uint16_t*)(wb + d->off[4 * l]);
      g.C = out; g.ldc = 2 * (int64_t)d->cout[l]; g.c_lo = d->cout[l];
      g.bias = (const float*)(wb + d->off[4 * l + 1]); g.scale = (const float*)(wb + d->off[4 * l + 2]); g.shift = (const float*)(wb + d->off[4 * l + 3]);
      g.M = M; g.N = d->cout[l]; g.Cin = d->cin[l]; g.taps = d->kernel[l]; g.dil = d->dilation[l]; g.T = T; g.flags = SDK_GEMM_RELU;
      if (int rc = sdk_conv_gemm_hp(ctx, &g, stream)) return rc;
      in = out;
      ldin = 2 * (int64_t)d->cout[l];
      in_lo = d->cout[l];
    }
    if (int rc = hp_asp_stats(ctx, in, ldin, in_lo, B, T, Cl, stats, stream)) return rc;
  } else {
    for (int l = 0; l < d->n_frame_layers; ++l) {
      uint16_t* out = (l & 1) ? b1 : b0;
      sdk_conv_gemm_args g;
      memset(&g, 0, sizeof(g));
      g.A = in; g.lda = ldin; g.W = (const uint16_t*)(wb + d->off[4 * l]); g.C = out; g.ldc = d->cout[l];
      g.bias = (const float*)(wb + d->off[4 * l + 1]); g.scale = (const float*)(wb + d->off[4 * l + 2]); g.shift = (const float*)(wb + d->off[4 * l + 3]);
      g.M = M; g.N = d->cout[l]; g.Cin = d->cin[l]; g.taps = d->kernel[l]; g.dil = d->dilation[l]; g.T = T; g.flags = SDK_GEMM_RELU | (f16 ? SDK_GEMM_F16 : 0u);
      if (l == 0 && d->first_tap_pack) g.tap_pack = d->first_tap_pack;
      if (int rc = sdk_conv_gemm(ctx, &g, stream)) return rc;
      in = out;
      ldin = d->cout[l];
    }
    if (int rc = asp_stats_impl(ctx, in, ldin, B, T, Cl, stats, stream, f16)) return rc;
  }
  return sdk_rows_fc(ctx, stats, 2 * Cl, nullptr, nullptr, (const float*)(wb + d->off[60]), (const float*)(wb + d->off[61]), emb, d->embed_dim, B, 2 * Cl,
                     d->embed_dim, 0, stream);
}

// ------------------------------------------------------------------------------ ResNet34 forward
// The WeSpeaker ResNet34 (the PyAnnote 3.1 speaker embedding): one sdk_resnet_conv2d per conv (a downsampling block's projection shortcut
// rides in its conv2's K), the temporal statistics pooling, and the embedding layer on sdk_rows_fc (fp32).
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
int rn_trunk(sdk_ctx* ctx, const char* wb, const sdk_resnet_desc* d, const uint16_t* feats, int ldf, int B, int T, uint16_t* const* buf,
             const uint16_t** last, int* Fl, int* Tlast, int* Cl, void* stream) {
  const bool f16 = d->precision == 2;
  const uint32_t fl = SDK_GEMM_RELU | (f16 ? SDK_GEMM_F16 : 0u);
  auto Wp = [&](int i) { return (const uint16_t*)(wb + d->off[2 * i]); };
  auto Bp = [&](int i) { return (const float*)(wb + d->off[2 * i + 1]); };
  uint16_t *X = buf[0], *H = buf[1], *Y = buf[2];
  sdk_resnet_conv_args a;
  memset(&a, 0, sizeof(a));
  a.x = feats; a.ldx = ldf; a.W = Wp(0); a.bias = Bp(0); a.y = X;
  a.B = B; a.F = d->n_feats; a.T = T; a.Cin = 1; a.Cout = d->width[0]; a.stride = 1; a.flags = fl;
  if (int rc = sdk_resnet_conv2d(ctx, &a, stream)) return rc;
  int F = d->n_feats, Tl = T, C = d->width[0], conv = 1;
  for (int l = 0; l < 4; ++l) {
    for (int j = 0; j < d->blocks[l]; ++j) {
      const int s = (j == 0 && l > 0) ? 2 : 1, Cw = d->width[l];
      const int Fo = rn_out(F, s), To = rn_out(Tl, s);
      const bool proj = j == 0 && (s != 1 || C != Cw);
      memset(&a, 0, sizeof(a));                                  // conv1 -> BN -> ReLU
      a.x = X; a.W = Wp(conv); a.bias = Bp(conv); a.y = H;
      a.B = B; a.F = F; a.T = Tl; a.Cin = C; a.Cout = Cw; a.stride = s; a.flags = fl;
      if (int rc = sdk_resnet_conv2d(ctx, &a, stream)) return rc;
      memset(&a, 0, sizeof(a));                                  // conv2 -> BN (+ projection shortcut in K | + identity) -> ReLU
      a.x = H; a.W = Wp(conv + 1); a.bias = Bp(conv + 1); a.y = Y;
      a.B = B; a.F = Fo; a.T = To; a.Cin = Cw; a.Cout = Cw; a.stride = 1; a.flags = fl;
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
  SDK_REQUIRE_WS("sdk_resnet_forward", "sdk_resnet_workspace_bytes", ws, ws_bytes, sdk_resnet_workspace_bytes(d, B, T), 256);
  SDK_REQUIRE(((uintptr_t)wblob % 256) == 0, "sdk_resnet_forward: wblob=%p must be 256-byte aligned", wblob);
  RnWs rw;
  rn_carve({(char*)ws, 0}, d, B, T, 1, &rw);
  uint16_t* const* buf = rw.buf;
  float* const stats = rw.stats;
  const char* wb = (const char*)wblob;
  const uint16_t* X;
  int F, Tl, C;
  if (int rc = rn_trunk(ctx, wb, d, feats, ldf, B, T, buf, &X, &F, &Tl, &C, stream)) return rc;
  if (int rc = resnet_tstp_impl(ctx, X, B, F, Tl, C, stats, stream, d->precision == 2)) return rc;
  return sdk_rows_fc(ctx, stats, 2 * C * F, nullptr, nullptr, (const float*)(wb + d->off[66]), (const float*)(wb + d->off[67]), emb, d->embed_dim, B,
                     2 * C * F, d->embed_dim, 0, stream);
}

extern "C" int sdk_resnet_forward_masked(sdk_ctx* ctx, const void* wblob, const sdk_resnet_desc* d, const uint16_t* feats, int ldf, int B, int T,
                                         int S, const float* w, const int32_t* valid, void* ws, size_t ws_bytes, float* emb, void* stream) {
  SDK_REQUIRE(ctx && wblob && feats && w && valid && ws && emb, "sdk_resnet_forward_masked: null argument");
  if (int rc = check_rdesc(d)) return rc;
  SDK_REQUIRE(B > 0 && T >= 9 && (int64_t)B * T < (1ll << 31), "sdk_resnet_forward_masked: bad batch (B=%d T=%d; segments need >= 9 frames)", B, T);
  SDK_REQUIRE(S >= 1 && (int64_t)B * S < (1ll << 31), "sdk_resnet_forward_masked: S=%d weight rows per segment (B=%d)", S, B);
  SDK_REQUIRE(ldf >= d->n_feats, "sdk_resnet_forward_masked: ldf=%d < feature width %d", ldf, d->n_feats);
  SDK_REQUIRE_WS("sdk_resnet_forward_masked", "sdk_resnet_masked_workspace_bytes", ws, ws_bytes, sdk_resnet_masked_workspace_bytes(d, B, T, S), 256);
  SDK_REQUIRE(((uintptr_t)wblob % 256) == 0, "sdk_resnet_forward_masked: wblob=%p must be 256-byte aligned", wblob);
  RnWs rw;
  rn_carve({(char*)ws, 0}, d, B, T, S, &rw);
  uint16_t* const* buf = rw.buf;
  float* const stats = rw.stats;
  const char* wb = (const char*)wblob;
  const uint16_t* X;
  int F, Tl, C;
  if (int rc = rn_trunk(ctx, wb, d, feats, ldf, B, T, buf, &X, &F, &Tl, &C, stream)) return rc;
  if (int rc = resnet_masked_tstp_impl(ctx, X, B, F, Tl, C, S, w, valid, stats, stream, d->precision == 2)) return rc;
  if (int rc = sdk_rows_fc(ctx, stats, 2 * C * F, nullptr, nullptr, (const float*)(wb + d->off[66]), (const float*)(wb + d->off[67]), emb, d->embed_dim,
                           B * S, 2 * C * F, d->embed_dim, 0, stream)) return rc;
  return resnet_zero_invalid_impl(ctx, emb, B * S, d->embed_dim, valid, stream);
}

// ------------------------------------------------------------------------------ centroid-linkage agglomerative clustering (ahc.hip)
namespace {
constexpr int AHC_MAX_N = 65536;    // the condensed distance count of one problem stays under 2^31
constexpr int AHC_MAX_DIM = 2048;
// the host-side refusals shared by both entry points: 0 = the offsets describe G problems the kernels serve
int check_ahc_offsets(const char* fn, const int32_t* offsets, int G, int dim) {
  SDK_REQUIRE(offsets, "%s: offsets is null", fn);
  SDK_REQUIRE(G >= 1, "%s: G=%d (at least one problem)", fn, G);
  SDK_REQUIRE(dim >= 1 && dim <= AHC_MAX_DIM, "%s: dim=%d (served: 1 .. %d)", fn, dim, AHC_MAX_DIM);
  SDK_REQUIRE(offsets[0] == 0, "%s: offsets[0]=%d (the first problem starts at row 0)", fn, offsets[0]);
  for (int g = 0; g < G; ++g) {
    const int64_t n = (int64_t)offsets[g + 1] - offsets[g];
    SDK_REQUIRE(n >= 1, "%s: offsets not increasing at problem %d (offsets[%d]=%d, offsets[%d]=%d: every problem needs a row)", fn, g, g, offsets[g],
                g + 1, offsets[g + 1]);
    SDK_REQUIRE(n <= AHC_MAX_N, "%s: problem %d has n=%lld rows (at most %d)", fn, g, (long long)n, AHC_MAX_N);
  }
  return 0;
}
}  // namespace

extern "C" size_t sdk_centroid_linkage_workspace_bytes(const int32_t* offsets, int G, int dim) {
  if (check_ahc_offsets("sdk_centroid_linkage_workspace_bytes", offsets, G, dim)) return 0;
  return ahc_workspace_bytes(offsets, G);
}

extern "C" int sdk_centroid_linkage(sdk_ctx* ctx, const float* E, int ldE, int dim, const int32_t* offsets, int G, double* Z, int32_t* status,
                                    void* workspace, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx && E && Z && status && workspace, "sdk_centroid_linkage: null argument (ctx=%p E=%p Z=%p status=%p workspace=%p)", (void*)ctx,
              (const void*)E, (void*)Z, (void*)status, workspace);
  if (int rc = check_ahc_offsets("sdk_centroid_linkage", offsets, G, dim)) return rc;
  SDK_REQUIRE(ldE >= dim, "sdk_centroid_linkage: ldE=%d < dim=%d", ldE, dim);
  SDK_REQUIRE((uintptr_t)E % 4 == 0 && (uintptr_t)Z % 8 == 0 && (uintptr_t)status % 4 == 0 && (uintptr_t)workspace % 256 == 0,
              "sdk_centroid_linkage: misaligned pointer (E=%p needs 4, Z=%p needs 8, status=%p needs 4, workspace=%p needs 256 bytes)",
              (const void*)E, (void*)Z, (void*)status, workspace);
  SDK_REQUIRE_WS("sdk_centroid_linkage", "sdk_centroid_linkage_workspace_bytes", workspace, ws_bytes, ahc_workspace_bytes(offsets, G), 1);
  return ahc_launch(ctx, E, ldE, dim, offsets, G, Z, status, workspace, stream);
}

// ------------------------------------------------------------------------------ linked centroid linkage (ahc.hip, the LINK kernels)
extern "C" size_t sdk_linked_linkage_workspace_bytes(const int32_t* offsets, int G, int dim) {
  if (check_ahc_offsets("sdk_linked_linkage_workspace_bytes", offsets, G, dim)) return 0;
  return ahc_workspace_bytes(offsets, G);
}

extern "C" int sdk_linked_linkage(sdk_ctx* ctx, const float* E, int ldE, int dim, const int32_t* group, const int32_t* offsets, int G, double stop,
                                  double* Z, int32_t* merges, int32_t* status, void* workspace, size_t ws_bytes, void* stream) {
  SDK_REQUIRE(ctx && E && group && Z && merges && status && workspace,
              "sdk_linked_linkage: null argument (ctx=%p E=%p group=%p Z=%p merges=%p status=%p workspace=%p)", (void*)ctx, (const void*)E,
              (const void*)group, (void*)Z, (void*)merges, (void*)status, workspace);
  if (int rc = check_ahc_offsets("sdk_linked_linkage", offsets, G, dim)) return rc;
  SDK_REQUIRE(ldE >= dim, "sdk_linked_linkage: ldE=%d < dim=%d", ldE, dim);
  SDK_REQUIRE(stop >= 0.0, "sdk_linked_linkage: stop=%g (a distance >= 0, or +inf for every allowed merge)", stop);     // false for a NaN too
  SDK_REQUIRE((uintptr_t)E % 4 == 0 && (uintptr_t)group % 4 == 0 && (uintptr_t)Z % 8 == 0 && (uintptr_t)merges % 4 == 0 && (uintptr_t)status % 4 == 0 &&
                  (uintptr_t)workspace % 256 == 0,
              "sdk_linked_linkage: misaligned pointer (E=%p needs 4, group=%p needs 4, Z=%p needs 8, merges=%p needs 4, status=%p needs 4, workspace=%p "
              "needs 256 bytes)", (const void*)E, (const void*)group, (void*)Z, (void*)merges, (void*)status, workspace);
  SDK_REQUIRE_WS("sdk_linked_linkage", "sdk_linked_linkage_workspace_bytes", workspace, ws_bytes, ahc_workspace_bytes(offsets, G), 1);
  return link_launch(ctx, E, ldE, dim, group, offsets, G, stop, Z, merges, status, workspace, stream);
}
