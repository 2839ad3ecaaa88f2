// The workgroup min / max reduction and the uint8 quantisation shared by the kernels that turn float
// images into model inputs (analyze2d.hip: reconstructions; baselines2d.hip: pixel-domain masked images
// and the CAM's float64 extrema; evaluate1d.hip: the reduction alone, for the peak normalisation).
#pragma once
#include "kernels.hpp"

// What block_reduce combines: a minimum, a maximum (float or double), or both at once as a MinMax pair.
template <class T>
struct MinMax {
  T mn, mx;
};
struct MinOp {  // fmin / fmax of two floats are fminf / fmaxf
  template <class T> __device__ T operator()(T a, T b) const { return fmin(a, b); }
};
struct MaxOp {
  template <class T> __device__ T operator()(T a, T b) const { return fmax(a, b); }
};
struct MinMaxOp {
  template <class T> __device__ MinMax<T> operator()(MinMax<T> a, MinMax<T> b) const {
    return {fmin(a.mn, b.mn), fmax(a.mx, b.mx)};
  }
};
template <class T> __device__ __forceinline__ T wave_xor(T v, int s) { return __shfl_xor(v, s, 64); }
template <class T> __device__ __forceinline__ MinMax<T> wave_xor(MinMax<T> v, int s) {
  return {__shfl_xor(v.mn, s, 64), __shfl_xor(v.mx, s, 64)};
}

// op over the workgroup: a wave-64 xor butterfly, one slot of `red` (LDS, blockDim.x / 64 <= 16 slots)
// per wave, a serial combine over the waves in order. Every thread of the block calls it and gets the
// result; the leading barrier lets a kernel call it again on the same `red`.
template <class V, class Op>
__device__ __forceinline__ V block_reduce(V v, Op op, V* red) {
  for (int s = 32; s > 0; s >>= 1) v = op(v, wave_xor(v, s));
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();  // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  v = red[0];
  for (int i = 1; i < nw; ++i) v = op(v, red[i]);
  return v;
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
