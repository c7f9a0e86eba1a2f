// What the loss kernels share: the reproducible workgroup sum and the smooth-L1 element.
#pragma once
#include <cmath>

#include "dtc_common.h"
#include "wave_ops.h"

#include "../../../include/detectorch_loss_hip.h"

namespace dtc {

constexpr int kLossThreads = 256;
constexpr int kLossWaves = kLossThreads / 64;
constexpr int kLossMaxBlocks = 1024;          // workgroups of one pass = partial results for the last sum

// Sum of v over the workgroup in a FIXED order (xor butterfly inside each wavefront: every lane ends with the same bits; then the
// wavefronts' sums in wave order): the total in every thread.  `sh`: kLossWaves slots of LDS, free to reuse after the call.
template <typename T> __device__ __forceinline__ T block_sum(T v, T* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();                              // (the slots may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = sh[0];
#pragma unroll
  for (int w = 1; w < kLossWaves; w++) t += sh[w];
  return t;
}

// lib/model/loss.py:14-20 for one element, evaluated in double from the float32 inputs (x = (pred - target) * alpha_in is exact to
// the last bit of a double).  beta: the float32 argument widened.  -> the loss term BEFORE the division by the row count;
// *slope = d term / d pred = (|x| <= beta ? x / beta : sign(x)) * alpha_in * alpha_out.
__device__ __forceinline__ double smooth_l1_term(float pred, float target, float alpha_in, float alpha_out, double beta,
                                                 double* slope) {
  const double x = ((double)pred - (double)target) * (double)alpha_in;
  const double ax = fabs(x);
  const bool quad = ax <= beta;                                                        // :18 torch.le: inclusive
  *slope = (quad ? x / beta : (x > 0.0 ? 1.0 : -1.0)) * (double)alpha_in * (double)alpha_out;
  return (quad ? 0.5 * x * x / beta : ax - 0.5 * beta) * (double)alpha_out;            // :16, :17, :20
}

}  // namespace dtc
