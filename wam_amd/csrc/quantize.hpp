// The uint8 quantisation shared by the kernels that turn float images into model inputs
// (analyze2d.hip: reconstructions; baselines2d.hip: pixel-domain masked images).
#pragma once
#include "kernels.hpp"

// min / max over the workgroup: wave-64 shuffles, one LDS step. Every thread of the block calls it.
__device__ __forceinline__ void block_minmax(float& mn, float& mx) {
  __shared__ float smn[16], smx[16];
  for (int s = 32; s > 0; s >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, s, 64));
    mx = fmaxf(mx, __shfl_xor(mx, s, 64));
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smn[w] = mn;
    smx[w] = mx;
  }
  __syncthreads();
  mn = smn[0];
  mx = smx[0];
  for (int i = 1; i < nw; ++i) {
    mn = fminf(mn, smn[i]);
    mx = fmaxf(mx, smx[i]);
  }
}

// RULE 0: normalize_data (src/evaluation_helpers.py:433-435) -> (x * 255).astype(uint8): min-max,
// values in [0, 255], truncation. A constant image (e.g. insertion step 0: all coefficients masked, a
// zero reconstruction) gives 0 / 0 = NaN, which numpy's NaN -> uint8 cast turns into 0 on x86
// (cvttss2si's 0x80000000, low byte 0): pinned here explicitly rather than left to the hardware's
// float -> int conversion of NaN.
// RULE 1: the analyzer's ((x - mn) / mx - mn) * 255 (src/analyzers.py:155; the precedence is the
// reference's), every step a float32 round-to-nearest operation in numpy's order, then numpy's
// float32 -> uint8 cast as x86 does it: truncation toward zero to int32, the low 8 bits kept (-3.7 ->
// 253, 300.7 -> 44); NaN and values outside int32 give cvttss2si's 0x80000000, so 0. Pinned
// explicitly too: the hardware's own conversion saturates.
template <int RULE>
__device__ __forceinline__ uint8_t quantize_one(float x, float mn, float mx) {
  if (RULE == 0) {
    const float s = __fmul_rn(__fdiv_rn(x - mn, mx - mn), 255.f);
    return (s != s) ? (uint8_t)0 : (uint8_t)(int)s;
  }
  const float s = __fmul_rn(__fsub_rn(__fdiv_rn(__fsub_rn(x, mn), mx), mn), 255.f);
  if (!(fabsf(s) < 2147483648.f)) return 0;  // NaN, +-inf, beyond int32
  return (uint8_t)((int)s & 255);
}

// ToTensor + Normalize of a quantised byte: (q / 255 - mean) / std, two IEEE divisions
__device__ __forceinline__ float normalize_byte(int q, float mean, float std) {
  return __fdiv_rn(__fdiv_rn((float)q, 255.f) - mean, std);
}
