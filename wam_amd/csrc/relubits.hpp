// The packed ReLU mask format shared by its producers and consumers (model_ew.hip, model_pw.hip):
// uint8 [n / 8], bit i % 8 of byte i / 8 is out[i] > 0 on the stored bf16 value, i the flat index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the mask byte of 8 stored bf16 values (a 16-byte vector): bit i is set when pattern i lies in
// [0x0001, 0x7f80] -- +0, -0, negatives and NaN give 0, denormals and +inf give 1
__device__ __forceinline__ uint32_t wam_pos_bits(const uint4& r) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m |= (uint32_t)(((w[k] & 0xffffu) - 1u) < 0x7f80u) << (2 * k);
    m |= (uint32_t)(((w[k] >> 16) - 1u) < 0x7f80u) << (2 * k + 1);
  }
  return m;
}
