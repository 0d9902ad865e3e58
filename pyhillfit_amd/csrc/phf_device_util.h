// phf_device_util.h — the small device and host-launch helpers the streaming analyses share (each was once pasted per .hip file).
#ifndef PHF_DEVICE_UTIL_H
#define PHF_DEVICE_UTIL_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "phf_common.h"

// a point's tag into [0, hi], a problem's point count into [0, stride]: the kernels index with them whatever the caller stored
__device__ inline int clamp_tag(int t, int hi) { return t < 0 ? 0 : (t > hi ? hi : t); }
__device__ inline int clamp_count(int n, int stride) { return n < 0 ? 0 : (n > stride ? stride : n); }

// sum over the wavefront by a fixed butterfly (a + b == b + a: every lane holds the same sum)
__device__ inline double wave_sum(double v) {
  _Pragma("unroll")
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block reductions through a small LDS array (blockDim.x <= 1024: 16 wavefronts)
__device__ inline double block_min(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v = __builtin_fmin(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x / 64] = v;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < (int)blockDim.x / 64; ++w) r = __builtin_fmin(r, sh[w]);
  return r;
}

__device__ inline double block_max(double v, double* sh) { return -block_min(-v, sh); }

__device__ inline unsigned block_min_u(unsigned v, unsigned* sh) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x / 64] = v;
  __syncthreads();
  unsigned r = sh[0];
  for (int w = 1; w < (int)blockDim.x / 64; ++w) r = sh[w] < r ? sh[w] : r;
  return r;
}

// workgroups of per_block units that cover n units
inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// a kernel that takes more than 64 KiB of dynamic LDS has to be allowed it once
template <typename K>
int allow_lds(K kernel, size_t bytes, const char* who) {
  if (bytes <= 65536) return PHF_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return phf_check_launch(who);
  return PHF_OK;
}

#endif  // PHF_DEVICE_UTIL_H
