// Wave64 / workgroup reduction helpers shared by the kernel files (DPP row operations, fixed summation order).
// Blocks are 256 threads (four wavefronts) wherever block_sum / block_max are used.
#pragma once
#include <hip/hip_runtime.h>

// threads per block of the kernel files that include this header (one that states it again must state the same value: the
// compiler warns about any other)
#define TPB 256
// streamed-once operands (matrix values / columns of the AMG sweeps): non-temporal loads keep them from evicting the
// gathered vector entries out of the 32 KB L1
#define NTLOAD(p) __builtin_nontemporal_load(p)

// ---------------------------------------------------------------- wave-level helpers
template <int CTRL>
__device__ __forceinline__ double dpp_shuffle(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// sum over aligned groups of 8 lanes (result in every lane of the group)
__device__ __forceinline__ double group8_sum(double v) {
  v += dpp_shuffle<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_shuffle<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_shuffle<0x141>(v);  // row_half_mirror
  return v;
}
// sum over aligned groups of 4 lanes
__device__ __forceinline__ double quad_sum(double v) {
  v += dpp_shuffle<0xB1>(v);  // quad_perm [1,0,3,2]
  v += dpp_shuffle<0x4E>(v);  // quad_perm [2,3,0,1]
  return v;
}
__device__ __forceinline__ double readlane_d(double v, int lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// sum over the 64 lanes of the wave (result in every lane)
__device__ __forceinline__ double wave_sum(double v) {
  v = group8_sum(v);
  v += dpp_shuffle<0x140>(v);  // row_mirror -> sums of 16
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
// maximum that keeps a NaN: fmax returns the other operand, which turned the inf-norm of a NaN field into 0.  For two numbers
// the result is fmax's, bit for bit.
__device__ __forceinline__ double max_nan(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }
__device__ __forceinline__ double wave_max(double v) {
  v = max_nan(v, dpp_shuffle<0xB1>(v));
  v = max_nan(v, dpp_shuffle<0x4E>(v));
  v = max_nan(v, dpp_shuffle<0x141>(v));
  v = max_nan(v, dpp_shuffle<0x140>(v));
  return max_nan(max_nan(readlane_d(v, 0), readlane_d(v, 16)), max_nan(readlane_d(v, 32), readlane_d(v, 48)));
}
// block (256 threads) sum; result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *sh /*[4]*/) {
  v = wave_sum(v);
  int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ double block_max(double v, double *sh) {
  v = wave_max(v);
  int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double r = max_nan(max_nan(sh[0], sh[1]), max_nan(sh[2], sh[3]));
  __syncthreads();
  return r;
}

// The same two sums by a butterfly of lane exchanges (result in every lane / every thread).  Kept apart from wave_sum / block_sum:
// those add in another order, and the functionals of the generic elements (L2 norms, fluxes, drag and lift), which have always
// been reduced this way, would change in their last bits.
__device__ __forceinline__ double wave_sum_xor(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ double block_sum_xor(double v, double *sh /*[4]*/) {
  v = wave_sum_xor(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
