// Weight-stationary expanding pointwise GEMM with the bottleneck block's elementwise neighbour as
// its epilogue.
//
//   D[M, N] = epilogue(X[M, K] . W[N, K]^T)      bf16 in, fp32 accumulate, one bf16 rounding
//
// X / D are NHWC activations viewed as [N*H*W, C]; W is the 1x1 convolution's weight as stored.
// The shapes are ResNet-50's conv3 of stages 2 and 3, (K, N) = (64, 256) and (128, 512): at
// KN / (K + N) = 51 and 102 flop/B they are streaming kernels (ridge ~400 flop/B), so the kernel's
// job is to keep HBM busy and to spare the pass that follows the GEMM today:
//   PW_TAIL  out = max((acc + ba[n]) + (s[m, n] + bs[n]), 0)     k_add_bias_relu on the accumulator
//   PW_MASK  out = y[m, n] > 0 ? acc (+ g2[m, n]) : 0            k_relu_mask on the accumulator
// With WAM_PW_ROUNDED acc is first rounded to bf16, the value the two-kernel path (bf16 GEMM, then
// the elementwise kernel) hands on: the model uses this form, so its results are those of that path
// (the c2 bench maps bit for bit), where the unrounded form moves them by 8e-2 relative L2.
//
// Structure
//   * W (this workgroup's N / NS rows of it) is resident in LDS, rows padded by 16 bytes so that
//     the ds_read_b128 fragment reads are conflict-free; workgroups are persistent and stride over
//     M tiles, so W is read once per workgroup.
//   * A wave owns 32 rows of M. Its X rows go from global memory straight into MFMA fragments
//     (16-byte loads, 8 consecutive k per lane); X never touches LDS.
//   * v_mfma_f32_32x32x16_bf16 with W as the A operand and X as the B operand: the accumulator is
//     D^T, lane (l & 31) owns pixel m and register r the channel (r & 3) + 8 (r >> 2) + 4 (l >> 5).
//     One v_permlane32_swap per register pair gives every lane 8 consecutive channels, so the
//     s / y / g2 reads and the D stores are 16-byte accesses along the channel axis.
//   * N is walked in 64-column chunks. The chunks' s / y / g2 operands sit in a ring of D register
//     buffers: a buffer is reloaded with the chunk D ahead (of this tile or the next) as soon as
//     its epilogue has consumed it, and the next tile's X rows load under the tile's last
//     epilogue, so D - 1 chunks of reads are in flight per wave across the MFMAs and the stores.
//   * K = 64: 37 KB of W, three workgroups of 4 waves per CU. K = 128: 136 KB of W, one workgroup
//     of 8 waves per CU (splitting N over two workgroups re-reads X and measured 20 % slower).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "relubits.hpp"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// f2bf(f < 0 ? 0 : f): the ReLU as one signed integer max on the rounded pattern (a value below zero
// keeps its sign bit through the rounding); NaN of either sign stays NaN, where fmaxf(f, 0) returns 0
__device__ __forceinline__ uint16_t f2bf_relu(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)((uint32_t)max((int32_t)u, 0) >> 16);
}
__device__ __forceinline__ float bf2f(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

__device__ __forceinline__ void unpack8(const uint4& r, float (&v)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = __uint_as_float(w[k] << 16);
    v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = (uint32_t)f2bf(v[2 * k]) | ((uint32_t)f2bf(v[2 * k + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint4 pack8_relu(const float (&v)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = (uint32_t)f2bf_relu(v[2 * k]) | ((uint32_t)f2bf_relu(v[2 * k + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}


constexpr int PW_TAIL = WAM_PW_TAIL, PW_MASK = WAM_PW_MASK;

// HAS_G2: PW_MASK with a second gradient. r0 = s (TAIL) / g2 (MASK), r1 = y (MASK).
// BITS (WAM_PW_BITS): `bits` is the packed ReLU mask, one bit per element of [M, N] -- written from
// the stored output in PW_TAIL, read in place of y in PW_MASK (r1 is then unused). A pixel's 64-column
// chunk is 8 mask bytes, of which lane half h holds bytes 2 j + h: the halves are combined so that
// the mask moves as one 8-byte access per pixel and chunk. (Collecting a round of D chunks into one
// 16-byte store per lane, with the bit taken from the fp32 sum, was tried: 168 VGPRs and scratch at
// K = 64, so it is not used.)
template <int K, int N, int NS, int WAVES, int MINW, int D, int MODE, bool HAS_G2, bool BITS>
__global__ void __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(MINW)))
    k_pw_gemm(int64_t M, const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
              const uint16_t* __restrict__ ba, const uint16_t* __restrict__ bs, const uint16_t* __restrict__ r0,
              const uint16_t* __restrict__ r1, uint8_t* bits, uint16_t* __restrict__ out, int rounded) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NL = N / NS;      // this workgroup's columns
  constexpr int LDW = K + 8;      // LDS row of W in bf16 elements (16 bytes of padding)
  constexpr int KS = K / 16;      // MFMA k steps
  constexpr int TM = 32 * WAVES;  // rows of M per workgroup tile
  __shared__ __attribute__((aligned(16))) uint16_t sw[NL * LDW];
  __shared__ __attribute__((aligned(16))) float sb[2][NL];

  const int tid = threadIdx.x;
  const int n_base = blockIdx.y * NL;
  for (int i = tid; i < NL * (K / 8); i += WAVES * 64) {
    const int row = i / (K / 8), c = i % (K / 8);
    *reinterpret_cast<uint4*>(&sw[row * LDW + c * 8]) =
        *reinterpret_cast<const uint4*>(&w[(int64_t)(n_base + row) * K + c * 8]);
  }
  if (MODE == PW_TAIL)
    for (int i = tid; i < NL; i += WAVES * 64) {
      sb[0][i] = ba ? bf2f(ba[n_base + i]) : 0.f;
      sb[1][i] = bs ? bf2f(bs[n_base + i]) : 0.f;
    }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t tiles = (M + TM - 1) / TM;

  auto load_x = [&](int64_t tile, uint4 (&f)[KS]) {
    int64_t m = tile * TM + wave * 32 + r;
    m = m < M ? m : M - 1;  // ragged tile / no next tile: a valid row, never stored
    const uint16_t* p = x + m * K + h * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) f[ks] = *reinterpret_cast<const uint4*>(p + ks * 16);
  };

  constexpr int NCH = NL / 64;  // 64-column chunks
  static_assert(NCH % D == 0, "the operand ring holds a whole number of rounds per tile");
  // a chunk's epilogue operands: 4 x 16 bytes per tensor and lane, channel nc*64 + 16 j + 8 h
  // (with BITS the y operand is the pixel's 8 mask bytes of the chunk, the same in both lane halves)
  auto load_e = [&](int64_t o, uint4 (&e0)[4], uint4 (&e1)[4], uint2& eb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (MODE == PW_TAIL || HAS_G2) e0[j] = *reinterpret_cast<const uint4*>(r0 + o + j * 16);
      if (MODE == PW_MASK && !BITS) e1[j] = *reinterpret_cast<const uint4*>(r1 + o + j * 16);
    }
    if (MODE == PW_MASK && BITS) eb = *reinterpret_cast<const uint2*>(bits + (o >> 3) - h);
  };
  auto row_of = [&](int64_t tile) {
    const int64_t m = tile * TM + wave * 32 + r;
    return (m < M ? m : M - 1) * N + n_base + h * 8;  // past the end: a valid row, loaded and dropped
  };

  // ring of D chunk buffers: chunk c lives in buffer c % D and is reloaded with chunk c + D (of
  // this tile or the next) as soon as its epilogue has consumed it, so D - 1 chunks are in flight
  uint4 xf[KS], e0[D][4], e1[D][4];
  uint2 eb[D];
  if ((int64_t)blockIdx.x < tiles) {
    load_x(blockIdx.x, xf);
#pragma unroll
    for (int d = 0; d < D; ++d) load_e(row_of(blockIdx.x) + d * 64, e0[d], e1[d], eb[d]);
  }

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const bool live = tile * TM + wave * 32 + r < M;
    const int64_t row = row_of(tile), row_next = row_of(tile + gridDim.x);

#pragma unroll 1
    for (int nc0 = 0; nc0 < NCH; nc0 += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int nc = nc0 + d;
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
          const uint16_t* wp = &sw[(nc * 64 + t * 32 + r) * LDW + h * 8];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const uint4 a = *reinterpret_cast<const uint4*>(wp + ks * 16);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                             __builtin_bit_cast(bf16x8, xf[ks]), acc[t], 0, 0, 0);
          }
        }
        // the tile's last MFMA is issued: the next tile's X rows load under this chunk's epilogue
        if (d == D - 1 && nc0 + D == NCH) load_x(tile + gridDim.x, xf);
        uint4 res[4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            // registers 8p .. 8p+3 hold channels 16p + 4h + i, registers 8p+4 .. 8p+7 channels
            // 16p + 8 + 4h + i: swapping the upper half of the first with the lower half of the
            // second leaves lane half h with channels 16p + 8h + 0..7
            float v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const auto pr = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[t][8 * p + i]),
                                                                __float_as_uint(acc[t][8 * p + 4 + i]), false, false);
              v[i] = __uint_as_float(pr[0]);
              v[4 + i] = __uint_as_float(pr[1]);
            }
            if (rounded) {  // the two-kernel path's bf16 GEMM result
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = bf2f(f2bf(v[i]));
            }
            const int j = 2 * t + p;
            if constexpr (MODE == PW_TAIL) {
              const int cl = nc * 64 + j * 16 + h * 8;
              float sv[8];
              unpack8(e0[d][j], sv);
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = (v[i] + sb[0][cl + i]) + (sv[i] + sb[1][cl + i]);
              res[j] = pack8_relu(v);  // NaN propagates, as in k_add_bias_relu (fmaxf would return 0)
            } else {
              float yv[8], gv[8];
              if constexpr (BITS) {  // byte 2 j + h of the 8: bit i set = y > 0
                const uint32_t mb = (j < 2 ? eb[d].x : eb[d].y) >> (16 * (j & 1) + 8 * h);
#pragma unroll
                for (int i = 0; i < 8; ++i) yv[i] = (mb >> i) & 1u ? 1.f : 0.f;
              } else {
                unpack8(e1[d][j], yv);
              }
              if (HAS_G2) unpack8(e0[d][j], gv);
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = yv[i] > 0.f ? (HAS_G2 ? v[i] + gv[i] : v[i]) : 0.f;
              res[j] = pack8(v);
            }
          }
        const int nn = nc + D;
        load_e(nn < NCH ? row + nn * 64 : row_next + (nn - NCH) * 64, e0[d], e1[d], eb[d]);
        if (live) {
#pragma unroll
          for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(out + row + nc * 64 + j * 16) = res[j];
        }
        if constexpr (MODE == PW_TAIL && BITS) {
          // this lane's bytes 2 j + h; the swap hands every lane both halves' words of its pixel
          const uint32_t mine = wam_pos_bits(res[0]) | (wam_pos_bits(res[1]) << 8) | (wam_pos_bits(res[2]) << 16) |
                                (wam_pos_bits(res[3]) << 24);
          const auto pr = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);
          const uint32_t ev = pr[0], od = pr[1];  // bytes 0 2 4 6 and 1 3 5 7
          uint2 mk;
          mk.x = (ev & 0xffu) | ((od & 0xffu) << 8) | ((ev & 0xff00u) << 8) | ((od & 0xff00u) << 16);
          mk.y = ((ev >> 16) & 0xffu) | (((od >> 16) & 0xffu) << 8) | ((ev >> 24) << 16) | ((od >> 24) << 24);
          if (live && h == 0) *reinterpret_cast<uint2*>(bits + ((row + nc * 64) >> 3)) = mk;
        }
      }
    }
  }
#endif
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// resident workgroups the device holds: CUs x workgroups per CU
int resident_wgs(int per_cu) {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256 * per_cu;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus[dev] = n;
  }
  return cus[dev] * per_cu;
}

// MINW: waves per SIMD the register budget is held to; DT / DM2 / DM1: operand ring depth of the
// tail, mask + g2 and mask kernels
template <int K, int N, int NS, int WAVES, int PER_CU, int MINW, int DT, int DM2, int DM1>
int launch(int mode, int64_t M, const uint16_t* x, const uint16_t* w, const uint16_t* ba, const uint16_t* bs,
           const uint16_t* r0, const uint16_t* r1, uint8_t* bits, uint16_t* out, int rounded, int max_wgs,
           hipStream_t st) {
  const int64_t tiles = (M + 32 * WAVES - 1) / (32 * WAVES);
  int64_t gx = resident_wgs(PER_CU) / NS;
  if (max_wgs > 0) gx = max_wgs;
  if (gx > tiles) gx = tiles;
  if (gx < 1) gx = 1;
  const dim3 grid((unsigned)gx, NS), block(WAVES * 64);
#define WAM_PW_LAUNCH(DD, MODE_, G2, B) \
  hipLaunchKernelGGL((k_pw_gemm<K, N, NS, WAVES, MINW, DD, MODE_, G2, B>), grid, block, 0, st, M, x, w, ba, bs, r0, r1, \
                     bits, out, rounded)
  if (mode == PW_TAIL && bits) WAM_PW_LAUNCH(DT, PW_TAIL, false, true);
  else if (mode == PW_TAIL) WAM_PW_LAUNCH(DT, PW_TAIL, false, false);
  else if (r0 && bits) WAM_PW_LAUNCH(DM2, PW_MASK, true, true);
  else if (r0) WAM_PW_LAUNCH(DM2, PW_MASK, true, false);
  else if (bits) WAM_PW_LAUNCH(DM1, PW_MASK, false, true);
  else WAM_PW_LAUNCH(DM1, PW_MASK, false, false);
#undef WAM_PW_LAUNCH
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

}  // namespace

extern "C" {

int wam_pw_supported(int dtype, int64_t K, int64_t N) {
  return dtype == WAM_DT_BF16 && ((K == 64 && N == 256) || (K == 128 && N == 512));
}

int wam_pw_gemm_ex(int mode, int64_t M, int64_t K, int64_t N, const void* x, const void* w, const void* bias_a,
                   const void* bias_b, const void* r0, const void* r1, void* out, int max_workgroups, void* stream) {
  const int rounded = (mode & WAM_PW_ROUNDED) ? 1 : 0;
  // WAM_PW_BITS: r1 is the packed mask. The signature is pinned, so r1 stays `const void*` although
  // PW_TAIL WRITES the mask through it (include/wam_hip.h says so); the kernel gets it as the separate,
  // non-const and non-restrict `bits` pointer and a NULL r1.
  const bool packed = mode >= 0 && (mode & WAM_PW_BITS);
  if (mode >= 0) mode &= ~(WAM_PW_ROUNDED | WAM_PW_BITS);
  if (M <= 0 || !x || !w || !out || (mode != WAM_PW_TAIL && mode != WAM_PW_MASK) || max_workgroups < 0)
    return WAM_ERR_INVALID_ARG;
  if ((mode == WAM_PW_TAIL && (!r0 || (r1 != nullptr) != packed)) || (mode == WAM_PW_MASK && (!r1 || bias_a || bias_b)))
    return WAM_ERR_INVALID_ARG;
  if (!wam_pw_supported(WAM_DT_BF16, K, N)) return WAM_ERR_UNSUPPORTED;
  if (M > (int64_t(1) << 52)) return WAM_ERR_UNSUPPORTED;
  // the kernel moves 16 bytes per access; biases are read element by element
  for (const void* p : {x, w, r0, r1, (const void*)out})
    if (p && !al16(p)) return WAM_ERR_UNSUPPORTED;
  const uint16_t *xp = (const uint16_t*)x, *wp = (const uint16_t*)w, *ba = (const uint16_t*)bias_a,
                 *bs = (const uint16_t*)bias_b, *p0 = (const uint16_t*)r0, *p1 = packed ? nullptr : (const uint16_t*)r1;
  uint8_t* pb = packed ? (uint8_t*)r1 : nullptr;
  hipStream_t st = (hipStream_t)stream;
  uint16_t* op = (uint16_t*)out;
  // measured on MI355X (scripts/kbench_pointwise.py): K = 64 three workgroups of 4
  // waves per CU, K = 128 one workgroup of 8 waves holding all of W; operand ring as deep as the
  // registers allow without scratch
  if (K == 64) return launch<64, 256, 1, 4, 3, 3, 2, 2, 2>(mode, M, xp, wp, ba, bs, p0, p1, pb, op, rounded, max_workgroups, st);
  return launch<128, 512, 1, 8, 1, 2, 4, 2, 4>(mode, M, xp, wp, ba, bs, p0, p1, pb, op, rounded, max_workgroups, st);
}

int wam_pw_gemm(int mode, int dtype, int64_t M, int64_t K, int64_t N, const void* x, const void* w,
                const void* bias_a, const void* bias_b, const void* r0, const void* r1, void* out, void* stream) {
  if (dtype != WAM_DT_F32 && dtype != WAM_DT_BF16) return WAM_ERR_INVALID_ARG;
  if (dtype != WAM_DT_BF16) return WAM_ERR_UNSUPPORTED;
  return wam_pw_gemm_ex(mode, M, K, N, x, w, bias_a, bias_b, r0, r1, out, 0, stream);
}

}  // extern "C"
