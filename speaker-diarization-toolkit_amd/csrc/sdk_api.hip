// libsdk_hip.so: the last error, context, device memory, options and the profiler (the model forwards are forward_*.hip).
#include <stdarg.h>
#include <string.h>

#include "common.hpp"

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
