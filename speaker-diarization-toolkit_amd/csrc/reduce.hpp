// Wave and workgroup reductions shared by every kernel file (included from common.hpp; wave = 64 lanes).
//
// Every wave-level function is the xor butterfly over offsets 32, 16, .. 1: all 64 lanes return the result, and the order of the additions is
// the same in every lane and every run.  The whole wave must be active (uniform control flow).  The (value, index) reductions with their own
// tie and NaN rules, the scans and the half-wave exchanges stay in the files that use them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// float64: the addition is written __dadd_rn, so that no caller's multiply can be contracted into it, whatever -ffp-contract its file is built
// with.  It is the form tr_calib_kernel's sums were pinned with, and it was taken over `v += ..` because the compiler emits the same
// instructions for both: samples.hip, whose copy had `+=`, and trials.hip, whose copy had __dadd_rn, compile to the same device assembly
// as before with this one function (the shuffled operand is never a product, so there was nothing to contract).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the integers: int, uint32_t, unsigned long long (exact in any order; an unsigned sum wraps)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  static_assert(std::is_integral<T>::value, "float and double have their own overloads");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
  static_assert(std::is_integral<T>::value, "float and double have their own overloads");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// The workgroup's sum in a fixed tree: the butterfly inside each wave, then the waves' sums added in wave order, ((w0 + w1) + w2) + w3.  Every
// thread returns it, bit-identical run to run.
//   - blockDim.x is a multiple of 64 (the callers launch 64, 128 or 256 threads); s_red holds blockDim.x / 64 doubles.
//   - Uniform control flow: every thread of the workgroup calls it.  It synchronises (two barriers); the leading one frees s_red, so it may
//     be called again and again with the same scratch.
//   - The chain starts from s_red[0], not from 0.0: a sum whose every term is -0.0 stays -0.0.  No caller can tell: the norms of
//     plda_front.hpp, vbx_centroids_kernel, km_finish_kernel, stream_step_kernel and diarize_centroids_kernel go through sqrt into
//     fmax(.., 1e-300) or a `> 0.0` test (sqrt(-0.0) = -0.0 fails it as +0.0 does); snorm_select_kernel adds nk * t to it and divides, and its
//     terms start from +0.0, which no addition turns into -0.0; vbx_mstep_kernel's two sums end in `.. + 1.0` per term (never -0.0) and in
//     (invL + al^2) Phi[d] with invL > 0, and both are only ever added to other terms afterwards.
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = s_red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += s_red[w];
  return r;
}
