// Cross-scale statistics of WAM maps and top-p mask agreement (the fork's utils.py and the agreement
// measures of compare_iou_models.ipynb) on the GPU.
//
// wam_level_stats: per image, the diagonal blocks of get_diagonal (level j: rows and columns
// [size >> (j + 1), size >> j), approximation [0, size >> J)) are read once. k_level_abs sums |v|
// per block (get_gradients_attribution_on_levels' terms); k_level_var resizes every detail block to
// T x T with scipy.ndimage.zoom(order=1)'s arithmetic, restated in float64 operation by operation,
// and takes np.var over the levels per pixel. Both write per-workgroup partial sums to the caller's
// workspace and k_level_finish adds them in a fixed order: no floating-point atomics, the same bits
// on every call.
//
// wam_mask_iou: pixel x of map i is selected at q when maps[i, x] >= thr[i, q]. One __ballot per
// (map, q) turns a wave's 64 pixels into a 64-bit mask in LDS; lane l then owns the (q, pair)
// combinations l, l + 64, ... and counts popcount(a & b), popcount(a | b) into registers: two
// popcounts per 64 pixels instead of one read-modify-write per pixel. Integer counts are exact, so
// the per-workgroup flush uses integer atomics.
#include "kernels.hpp"

// The zoom and the variance follow scipy and numpy rounding by rounding: no multiply of this file may be
// fused into a following add (hipcc contracts across statements by default, also through __dmul_rn /
// __dadd_rn, which are plain operators in the headers).
#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------ level stats

constexpr int kAbsBlock = 256;
constexpr int kAbsPerWg = 512;   // elements of the finest block per workgroup (2 per thread)
constexpr int kAbsMaxParts = 64;
constexpr int kVarBlock = 64;    // one wave per workgroup: a single 112 x 112 map still gives 196 workgroups
constexpr int kFinBlock = 256;

struct LevelGeom {
  int size, J, T;
  double zoom[WAM_MAX_LEVELS];   // (n - 1) / (m - 1) of level j (1 when m == 1), divided on the host
};

__host__ __device__ __forceinline__ int level_start(int size, int J, int b) { return b < J ? size >> (b + 1) : 0; }
__host__ __device__ __forceinline__ int level_side(int size, int J, int b) {
  return b < J ? (size >> b) - (size >> (b + 1)) : size >> J;
}

int abs_parts(int size) {
  const int64_t n0 = level_side(size, 1, 0);
  const int64_t p = (n0 * n0 + kAbsPerWg - 1) / kAbsPerWg;
  return (int)(p < 1 ? 1 : (p > kAbsMaxParts ? kAbsMaxParts : p));
}
int64_t var_parts(int T) { return T > 0 ? ((int64_t)T * T + kVarBlock - 1) / kVarBlock : 0; }

// sum over the workgroup in a fixed order: xor tree inside each wave, then the waves in order
template <int BLOCK>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  if (BLOCK == 64) return v;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int i = 1; i < BLOCK / 64; ++i) t += red[i];
  return t;
}

// grid: x = part, y = block (J + 1), z = image. Part p owns elements [p * n^2 / P, (p + 1) * n^2 / P)
// of the block (row-major); a thread adds its elements in ascending order.
__global__ void __launch_bounds__(kAbsBlock) k_level_abs(int size, int J, const double* __restrict__ maps,
                                                         double* __restrict__ part) {
  __shared__ double red[kAbsBlock / 64];
  const int b = blockIdx.y, P = gridDim.x;
  const int64_t img = blockIdx.z;
  const int s = level_start(size, J, b), n = level_side(size, J, b);
  const uint32_t ne = (uint32_t)n * (uint32_t)n;  // < 2^31 (checked by the host): 32-bit index arithmetic
  const uint32_t e0 = (uint32_t)((uint64_t)ne * blockIdx.x / P), e1 = (uint32_t)((uint64_t)ne * (blockIdx.x + 1) / P);
  const double* m = maps + img * (int64_t)size * size;
  double acc = 0.0;
  for (uint32_t e = e0 + threadIdx.x; e < e1; e += kAbsBlock) {
    const uint32_t r = e / (uint32_t)n, c = e - r * (uint32_t)n;
    acc += fabs(m[(int64_t)(s + r) * size + s + c]);
  }
  acc = block_sum<kAbsBlock>(acc, red);
  if (threadIdx.x == 0) part[(img * (J + 1) + b) * P + blockIdx.x] = acc;
}

// scipy.ndimage.zoom(order=1, mode='constant', grid_mode=False) along one axis: output index o reads
// input coordinate cc = zoom * o (one rounded multiply). A coordinate above n - 1 -- the product can
// round one ulp over at the last index -- is out of bounds and the sample is cval = 0. The weights are
// w0 = 1 - (cc - floor(cc)) and w1 = 1 - w0 (scipy derives the last weight from the others); the tap
// at n, met only with cc == n - 1 and w1 == 0, is read at its mirror image n - 2, as scipy does.
struct Tap {
  int i0, i1;
  double w0, w1;
  bool in;
};
__device__ __forceinline__ Tap zoom_tap(double zoom, int o, int n) {
  Tap t;
  const double cc = zoom * (double)o;
  t.in = !(cc > (double)(n - 1));
  const double fl = floor(cc);
  t.i0 = t.in ? (int)fl : 0;
  t.i1 = t.i0 + 1 < n ? t.i0 + 1 : (n > 1 ? n - 2 : 0);
  t.w0 = 1.0 - (cc - fl);
  t.w1 = 1.0 - t.w0;
  return t;
}

// grid: x = chunks of kVarBlock output pixels, y = image. A thread owns one pixel of the T x T
// variance map: J zoomed values (constant indices: the loop is fully unrolled), np.var's
// mean((v - mean(v))^2) with numpy's left-to-right sums over the level axis.
__global__ void __launch_bounds__(kVarBlock) k_level_var(LevelGeom g, const double* __restrict__ maps,
                                                         double* __restrict__ var_map, double* __restrict__ part) {
  const int T = g.T, J = g.J, size = g.size;
  const int64_t img = blockIdx.y;
  const uint32_t px = blockIdx.x * kVarBlock + threadIdx.x;  // T^2 < 2^31 (checked by the host)
  const bool live = px < (uint32_t)T * (uint32_t)T;
  double var = 0.0;
  if (live) {
    const int r = (int)(px / (uint32_t)T), c = (int)(px - (uint32_t)r * (uint32_t)T);
    const double* m = maps + img * (int64_t)size * size;
    double v[WAM_MAX_LEVELS];
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < WAM_MAX_LEVELS; ++j) {
      v[j] = 0.0;
      if (j < J) {
        const int s = level_start(size, J, j), n = level_side(size, J, j);
        const Tap tr = zoom_tap(g.zoom[j], r, n), tc = zoom_tap(g.zoom[j], c, n);
        double t = 0.0;
        if (tr.in && tc.in) {
          const double* b0 = m + (int64_t)(s + tr.i0) * size + s;
          const double* b1 = m + (int64_t)(s + tr.i1) * size + s;
          t = t + (b0[tc.i0] * tr.w0) * tc.w0;
          t = t + (b0[tc.i1] * tr.w0) * tc.w1;
          t = t + (b1[tc.i0] * tr.w1) * tc.w0;
          t = t + (b1[tc.i1] * tr.w1) * tc.w1;
        }
        v[j] = t;
        sum = j == 0 ? t : sum + t;
      }
    }
    const double mean = sum / (double)J;
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < WAM_MAX_LEVELS; ++j) {
      if (j < J) {
        const double d = v[j] - mean;
        const double d2 = d * d;
        ss = j == 0 ? d2 : ss + d2;
      }
    }
    var = ss / (double)J;
    if (var_map) var_map[img * (int64_t)T * T + px] = var;
  }
  if (part) {
    const double tot = block_sum<kVarBlock>(var, nullptr);
    if (threadIdx.x == 0) part[img * (int64_t)gridDim.x + blockIdx.x] = tot;
  }
}

// one workgroup per image: thread b < J + 1 adds the P partials of block b in order; the variance
// partials are added strided per thread, then over the workgroup (block_sum), and divided by T^2
__global__ void __launch_bounds__(kFinBlock) k_level_finish(int J, int P, const double* __restrict__ abs_part,
                                                            double* __restrict__ abs_sums, int64_t VP, int T,
                                                            const double* __restrict__ var_part,
                                                            double* __restrict__ mean_var) {
  __shared__ double red[kFinBlock / 64];
  const int64_t img = blockIdx.x;
  if (abs_sums && (int)threadIdx.x <= J) {
    const double* p = abs_part + (img * (J + 1) + threadIdx.x) * P;
    double t = p[0];
    for (int i = 1; i < P; ++i) t += p[i];
    abs_sums[img * (J + 1) + threadIdx.x] = t;
  }
  if (mean_var) {
    const double* p = var_part + img * VP;
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < VP; i += kFinBlock) t += p[i];
    t = block_sum<kFinBlock>(t, red);
    if (threadIdx.x == 0) mean_var[img] = t / ((double)T * (double)T);
  }
}

// ------------------------------------------------------------------------------------- mask IoU

constexpr int kIouMaxM = 16, kIouMaxQ = 16;
constexpr int kIouMaxCombo = kIouMaxQ * (kIouMaxM * (kIouMaxM - 1) / 2);  // 1920
constexpr int kIouPerLane = kIouMaxCombo / 64;                              // 30
constexpr int kIouBlock = 256, kIouWaves = kIouBlock / 64;

// A workgroup owns `iters` consecutive chunks of 256 pixels, a wave 64 pixels of each chunk.
// LDS: tab[c] = (row of map i) | (row of map j) << 16 in the wave's mask table for combination
// c = q * pairs + pair -- also the index of the output counters; masks[wave][m * Q + q]; cnt[2][c].
__global__ void __launch_bounds__(kIouBlock) k_mask_iou(int M, int Q, int64_t len, const double* __restrict__ maps,
                                                        const double* __restrict__ thr, int64_t iters,
                                                        unsigned long long* __restrict__ inter,
                                                        unsigned long long* __restrict__ uni) {
  __shared__ unsigned long long masks[kIouWaves][kIouMaxM * kIouMaxQ];
  __shared__ uint32_t tab[kIouMaxCombo];
  __shared__ uint32_t cnt[2][kIouMaxCombo];
  const int pairs = M * (M - 1) / 2, ncombo = pairs * Q;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = threadIdx.x; c < ncombo; c += kIouBlock) {
    const int q = c / pairs;
    int rem = c - q * pairs, i = 0;
    while (rem >= M - 1 - i) {
      rem -= M - 1 - i;
      ++i;
    }
    const int j = i + 1 + rem;
    tab[c] = (uint32_t)(i * Q + q) | ((uint32_t)(j * Q + q) << 16);
    cnt[0][c] = 0;
    cnt[1][c] = 0;
  }
  uint32_t ai[kIouPerLane], au[kIouPerLane];
#pragma unroll
  for (int k = 0; k < kIouPerLane; ++k) ai[k] = au[k] = 0;
  __syncthreads();
  unsigned long long* mk = masks[wave];
  const int64_t chunk0 = (int64_t)blockIdx.x * iters;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t x = (chunk0 + it) * kIouBlock + threadIdx.x;
    for (int m = 0; m < M; ++m) {
      const double v = x < len ? maps[(int64_t)m * len + x] : (double)NAN;  // NaN >= t is false: never selected
      unsigned long long keep = 0;
      for (int q = 0; q < Q; ++q) {
        const unsigned long long b = __ballot(v >= thr[m * Q + q]);
        if (lane == q) keep = b;
      }
      if (lane < Q) mk[m * Q + lane] = keep;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kIouPerLane; ++k) {
      const int c = lane + 64 * k;
      if (c < ncombo) {
        const uint32_t t = tab[c];
        const unsigned long long a = mk[t & 0xffffu], b = mk[t >> 16];
        ai[k] += (uint32_t)__popcll(a & b);
        au[k] += (uint32_t)__popcll(a | b);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kIouPerLane; ++k) {
    const int c = lane + 64 * k;
    if (c < ncombo) {
      if (ai[k]) atomicAdd(&cnt[0][c], ai[k]);
      if (au[k]) atomicAdd(&cnt[1][c], au[k]);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ncombo; c += kIouBlock) {
    if (cnt[0][c]) atomicAdd(&inter[c], (unsigned long long)cnt[0][c]);
    if (cnt[1][c]) atomicAdd(&uni[c], (unsigned long long)cnt[1][c]);
  }
}

}  // namespace

extern "C" {

int64_t wam_level_stats_ws_bytes(int64_t images, int size, int levels, int target) {
  if (images < 0 || size < 1 || levels < 0 || levels > WAM_MAX_LEVELS || target < 0) return -1;
  return 8 * images * ((int64_t)(levels + 1) * abs_parts(size) + var_parts(target));
}

int wam_level_stats(int64_t images, int size, int levels, const double* maps, int target, const int32_t* out_len,
                    double* abs_sums, double* var_map, double* mean_var, void* ws, int64_t ws_bytes,
                    void* stream) {
  if (images < 0 || size < 1 || levels < 0 || levels > WAM_MAX_LEVELS || !maps) return WAM_ERR_INVALID_ARG;
  const bool want_var = var_map || mean_var;
  if (want_var && (levels < 1 || target < 1 || !out_len)) return WAM_ERR_INVALID_ARG;
  if (!want_var) target = 0;
  if (!abs_sums && !want_var) return WAM_OK;
  LevelGeom g{};
  g.size = size;
  g.J = levels;
  g.T = target;
  for (int j = 0; j < levels && want_var; ++j) {
    const int n = level_side(size, levels, j), m = out_len[j];
    if (n < 1) return WAM_ERR_INVALID_ARG;   // the reference divides by this side
    if (m < target) return WAM_ERR_SHAPE;    // the reference's np.stack fails on the short level
    g.zoom[j] = m > 1 ? (double)(n - 1) / (double)(m - 1) : 1.0;
  }
  if (images == 0) return WAM_OK;
  // the largest block side: level 0's, or the whole map when levels == 0 (the approximation block); target <= it
  const int64_t n0 = levels > 0 ? level_side(size, levels, 0) : size;
  if (n0 * n0 > INT32_MAX || (int64_t)target * target > INT32_MAX) return WAM_ERR_UNSUPPORTED;
  const int P = abs_parts(size);
  const int64_t VP = var_parts(target);
  if (!ws || ws_bytes < wam_level_stats_ws_bytes(images, size, levels, target)) return WAM_ERR_INVALID_ARG;
  double* abs_part = static_cast<double*>(ws);
  double* var_part = abs_part + images * (int64_t)(levels + 1) * P;
  hipStream_t st = (hipStream_t)stream;
  const int64_t map_len = (int64_t)size * size;
  double block_elems = 0.0, detail_elems = 0.0;
  for (int b = 0; b <= levels; ++b) {
    const double n = level_side(size, levels, b);
    block_elems += n * n;
    if (b < levels) detail_elems += n * n;
  }
  for (int64_t i0 = 0; i0 < images; i0 += 65535) {  // gridDim.y / .z hold 65535 images
    const int64_t ni = images - i0 < 65535 ? images - i0 : 65535;
    if (abs_sums) {
      WamTimer tm(st, "k_level_abs", 8.0 * ni * block_elems + 8.0 * ni * (levels + 1) * P);
      hipLaunchKernelGGL(k_level_abs, dim3(P, levels + 1, (unsigned)ni), dim3(kAbsBlock), 0, st, size, levels,
                         maps + i0 * map_len, abs_part + i0 * (levels + 1) * P);
      WAM_LAUNCH_CHECK();
    }
    if (want_var) {
      WamTimer tm(st, "k_level_var", 8.0 * ni * detail_elems + (var_map ? 8.0 * ni * target * target : 0.0) +
                                         (mean_var ? 8.0 * ni * VP : 0.0));
      hipLaunchKernelGGL(k_level_var, dim3((unsigned)VP, (unsigned)ni), dim3(kVarBlock), 0, st, g, maps + i0 * map_len,
                         var_map ? var_map + i0 * (int64_t)target * target : nullptr,
                         mean_var ? var_part + i0 * VP : nullptr);
      WAM_LAUNCH_CHECK();
    }
  }
  if (abs_sums || mean_var) {
    WamTimer tm(st, "k_level_finish", 8.0 * images * ((abs_sums ? (levels + 1) * (P + 1) : 0) + (mean_var ? VP + 1 : 0)));
    hipLaunchKernelGGL(k_level_finish, dim3((unsigned)(images < 1 ? 1 : images)), dim3(kFinBlock), 0, st, levels, P,
                       abs_part, abs_sums, VP, target, var_part, mean_var);
    WAM_LAUNCH_CHECK();
  }
  return WAM_OK;
}

void wam_mask_iou_limits(int* max_maps, int* max_q) {
  if (max_maps) *max_maps = kIouMaxM;
  if (max_q) *max_q = kIouMaxQ;
}

int wam_mask_iou(int M, int Q, int64_t len, const double* maps, const double* thr, uint64_t* inter, uint64_t* uni,
                 void* stream) {
  if (M < 2 || Q < 1 || len < 0 || !maps || !thr || !inter || !uni) return WAM_ERR_INVALID_ARG;
  if (M > kIouMaxM || Q > kIouMaxQ) return WAM_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int ncombo = Q * (M * (M - 1) / 2);
  WAM_HIP_CHECK(hipMemsetAsync(inter, 0, 8 * (size_t)ncombo, st));
  WAM_HIP_CHECK(hipMemsetAsync(uni, 0, 8 * (size_t)ncombo, st));
  if (len == 0) return WAM_OK;
  // chunks of 256 pixels; a workgroup takes enough of them that its flush (2 * ncombo integer
  // atomics) stays below one atomic per two pixels, and more when the map is longer than 4096 workgroups' worth
  const int64_t chunks = (len + kIouBlock - 1) / kIouBlock;
  int64_t iters = (ncombo + 63) / 64;
  if ((chunks + iters - 1) / iters > 4096) iters = (chunks + 4095) / 4096;
  if (iters * kIouBlock > (int64_t)1 << 31) return WAM_ERR_UNSUPPORTED;  // 32-bit counters per workgroup
  const int64_t grid = (chunks + iters - 1) / iters;
  WamTimer tm(st, "k_mask_iou", 8.0 * M * (double)len + 8.0 * M * Q + 16.0 * ncombo);
  hipLaunchKernelGGL(k_mask_iou, dim3((unsigned)grid), dim3(kIouBlock), 0, st, M, Q, len, maps, thr, iters,
                     reinterpret_cast<unsigned long long*>(inter), reinterpret_cast<unsigned long long*>(uni));
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

}  // extern "C"
