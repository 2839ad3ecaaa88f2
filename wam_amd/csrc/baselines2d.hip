// Pixel-domain baselines (EvalImageBaselines, src/evaluators.py:805-1180; GradCAM / GradCAMPlusPlus /
// SmoothGrad, src/evaluation_helpers.py:72-320): the methods WAM is compared against, scored with
// insertion, deletion and mu-fidelity on the image itself. Per image and per mask the reference
// builds a float64 mask on the host, multiplies it into the image, min-max normalises, casts to uint8,
// goes through PIL and the transform; its Grad-CAM adds one weighted activation plane per feature
// channel in a Python loop. Here the masks are never stored: the ranking (or the superpixel grid) goes
// straight to the quantised, normalised model inputs of every mask, and one workgroup per image does
// the whole CAM. The mask kernels are HBM-bound streaming passes (write 4 * M * channels * plane bytes
// per set for 4 * (channels + 1) * plane read).
#include "maskexpand.hpp"
#include "quantize.hpp"

namespace {

constexpr int kMaxIter = 4096;    // two [n_iter + 2] tables of bucket extrema in LDS: 32 KB
constexpr int kMaxSplits = 32;    // workgroups that share the pixels of one set in the extrema pass
constexpr int kCamLdsCap = 160 * 1024;
constexpr int kCamGroup = 4;      // channels a wave reduces side by side

// order-preserving map of a finite float to uint32, so that LDS integer atomics take float extrema
__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
constexpr uint32_t kEmptyMin = 0xffffffffu, kEmptyMax = 0u;  // the images of no finite float

// the first mask m with rank < thr(m): a pixel enters the kept set there (leaves it, under deletion)
// and stays. n_iter + 1: no mask (a rank outside [0, plane), not part of the contract).
__device__ __forceinline__ int first_mask(int32_t rank, int n_iter, int n_comp, int64_t plane) {
  if (rank < 0) return 0;
  if (rank >= plane) return n_iter + 1;
  if (n_comp == 0) return n_iter;
  const int m = rank / n_comp + 1;
  return m < n_iter ? m : n_iter;
}

// ---- pass 1: the extrema of all n_iter + 1 masked images of a set from one read of the image. Bucket
// b = first_mask collects the extrema of its pixels over all channels; mask m keeps the buckets <= m
// (insertion) or > m (deletion), so its extrema are a prefix (suffix) scan of the buckets, with 0
// joined in when a pixel is dropped: a dropped pixel is +-0.
// k_rank_extrema: workgroup (split, set) buckets its slice of the pixels in LDS (integer atomics on the
// ordered images of the floats) and stores its table, part [sets, splits, 2, n_iter + 2].
__global__ void __launch_bounds__(256) k_rank_extrema(int channels, int64_t plane, const float* __restrict__ img,
                                                      const int32_t* __restrict__ rank, int n_iter, int n_comp,
                                                      uint32_t* __restrict__ part) {
  __shared__ uint32_t smin[kMaxIter + 2], smax[kMaxIter + 2];
  const int nb = n_iter + 2;
  const int64_t s = blockIdx.y;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    smin[b] = kEmptyMin;
    smax[b] = kEmptyMax;
  }
  __syncthreads();
  const float* x = img + s * channels * plane;
  const int32_t* rk = rank + s * plane;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < plane; p += (int64_t)gridDim.x * blockDim.x) {
    float mn = x[p], mx = mn;
    for (int c = 1; c < channels; ++c) {
      const float v = x[c * plane + p];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
    const int b = first_mask(rk[p], n_iter, n_comp, plane);
    atomicMin(&smin[b], f2ord(mn));
    atomicMax(&smax[b], f2ord(mx));
  }
  __syncthreads();
  uint32_t* o = part + (s * gridDim.x + blockIdx.x) * 2 * nb;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    o[b] = smin[b];
    o[nb + b] = smax[b];
  }
}

// k_rank_scan, one workgroup per set: all threads join the splits' tables into LDS, then wave 0 scans the
// buckets in the order they join the kept set: j = b (insertion), n_iter + 1 - b (deletion).
// ext [sets, n_iter + 1, 2] = (mn, mx).
__global__ void __launch_bounds__(256) k_rank_scan(int splits, int n_iter, int deletion,
                                                   const uint32_t* __restrict__ part, float* __restrict__ ext) {
  __shared__ uint32_t smin[kMaxIter + 2], smax[kMaxIter + 2];
  const int nb = n_iter + 2;
  const int64_t s = blockIdx.x;
  const uint32_t* t = part + s * splits * 2 * nb;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    uint32_t a = kEmptyMin, z = kEmptyMax;
#pragma unroll 8
    for (int q = 0; q < splits; ++q) {
      a = min(a, t[q * 2 * nb + b]);
      z = max(z, t[q * 2 * nb + nb + b]);
    }
    smin[b] = a;
    smax[b] = z;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const bool del = deletion != 0;
  int jl = -1;  // the last bucket, in that order, that holds a pixel
  for (int j = lane; j < nb; j += 64)
    if (smax[del ? nb - 1 - j : j] != kEmptyMax) jl = j;
  for (int d = 32; d > 0; d >>= 1) jl = max(jl, __shfl_xor(jl, d, 64));
  uint32_t cmn = kEmptyMin, cmx = kEmptyMax;
  for (int j0 = 0; j0 < nb; j0 += 64) {
    const int j = j0 + lane;
    uint32_t a = kEmptyMin, z = kEmptyMax;
    if (j < nb) {
      a = smin[del ? nb - 1 - j : j];
      z = smax[del ? nb - 1 - j : j];
    }
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t ta = __shfl_up(a, d, 64), tz = __shfl_up(z, d, 64);
      if (lane >= d) {
        a = min(a, ta);
        z = max(z, tz);
      }
    }
    a = min(a, cmn);
    z = max(z, cmx);
    cmn = __shfl(a, 63, 64);
    cmx = __shfl(z, 63, 64);
    if (j <= n_iter) {  // buckets 0 .. j make up the kept set of mask m
      const int m = del ? n_iter - j : j;
      float mn = 0.f, mx = 0.f;
      if (a != kEmptyMin) {
        mn = ord2f(a);
        mx = ord2f(z);
        if (j < jl) {  // a later bucket holds a pixel: it is dropped here
          mn = fminf(mn, 0.f);
          mx = fmaxf(mx, 0.f);
        }
      }
      float* e = ext + (s * (n_iter + 1) + m) * 2;
      e[0] = mn;
      e[1] = mx;
    }
  }
}

// (q / 255 - mean[c]) / std[c] for the 256 bytes of each channel: the two divisions of ToTensor +
// Normalize are taken once per workgroup instead of once per pixel
__device__ __forceinline__ void fill_norm_lut(float (*lut)[256], int channels, const ChanNorm& cn) {
  if (threadIdx.x < 256) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < channels) lut[c][threadIdx.x] = normalize_byte((int)threadIdx.x, cn.mean[c], cn.std[c]);
  }
  __syncthreads();
}

// the three optional outputs of one masked value group (W = 4 consecutive pixels, or 1). Plain stores:
// streaming stores for `out` (the model reads it, no WAM kernel does) lost to them in the ranking pass
// and stayed within the spread in the superpixel pass (profiles/baselines_kbench.txt).
template <int W>
__device__ __forceinline__ void emit(const float* v, float mn, float mx, const float* lut, int64_t at,
                                     float* __restrict__ masked, uint8_t* __restrict__ u8, float* __restrict__ out) {
  uint8_t q[W];
#pragma unroll
  for (int i = 0; i < W; ++i) q[i] = quantize_one<0>(v[i], mn, mx);
  if constexpr (W == 4) {
    if (masked) *reinterpret_cast<wam_f4v*>(masked + at) = wam_f4v{v[0], v[1], v[2], v[3]};
    if (u8) *reinterpret_cast<uchar4*>(u8 + at) = make_uchar4(q[0], q[1], q[2], q[3]);
    if (out) *reinterpret_cast<wam_f4v*>(out + at) = wam_f4v{lut[q[0]], lut[q[1]], lut[q[2]], lut[q[3]]};
  } else {
    if (masked) masked[at] = v[0];
    if (u8) u8[at] = q[0];
    if (out) out[at] = lut[q[0]];
  }
}

// ---- pass 2: one thread owns W = 4 consecutive pixels of a set (1 on the scalar path): it reads their
// `channels` values and ranks once and writes them into the kMaskChunk masks of its blockIdx.y. For one
// mask and channel a wave writes 64 x 16 consecutive bytes of `out`.
template <int W>
__global__ void __launch_bounds__(256) k_rank_mask_pixels(int64_t sets, int channels, int64_t plane,
                                                          const float* __restrict__ img,
                                                          const int32_t* __restrict__ rank, int64_t n_iter,
                                                          int64_t n_comp, int deletion, ChanNorm cn,
                                                          const float* __restrict__ ext, float* __restrict__ masked,
                                                          uint8_t* __restrict__ u8, float* __restrict__ out) {
  __shared__ float lut[4][256];
  if (out) fill_norm_lut(lut, channels, cn);
  const int64_t M = n_iter + 1;
  const int64_t m0 = (int64_t)blockIdx.y * kMaskChunk;
  const int64_t m1 = m0 + kMaskChunk < M ? m0 + kMaskChunk : M;
  const bool del = deletion != 0;
  const int64_t units = plane / W;
  for (int64_t s = blockIdx.z; s < sets; s += gridDim.z) {
    const float* x = img + s * channels * plane;
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
      const int64_t e = u * W;
      float c[4][W];
      int32_t rk[W];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        if (ch >= channels) continue;
        if constexpr (W == 4) {
          const wam_f4v t = *reinterpret_cast<const wam_f4v*>(x + ch * plane + e);
          c[ch][0] = t.x, c[ch][1] = t.y, c[ch][2] = t.z, c[ch][3] = t.w;
        } else {
          c[ch][0] = x[ch * plane + e];
        }
      }
      if constexpr (W == 4) {
        const int4 t = *reinterpret_cast<const int4*>(rank + s * plane + e);
        rk[0] = t.x, rk[1] = t.y, rk[2] = t.z, rk[3] = t.w;
      } else {
        rk[0] = rank[s * plane + e];
      }
      for (int64_t m = m0; m < m1; ++m) {
        const int64_t thr = mask_thr(m, n_iter, n_comp, plane);
        const float mn = ext[(s * M + m) * 2], mx = ext[(s * M + m) * 2 + 1];
        float k[W];
#pragma unroll
        for (int i = 0; i < W; ++i) k[i] = (((int64_t)rk[i] < thr) != del) ? 1.f : 0.f;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
          if (ch >= channels) continue;
          float v[W];
#pragma unroll
          for (int i = 0; i < W; ++i) v[i] = c[ch][i] * k[i];
          emit<W>(v, mn, mx, lut[ch], ((s * M + m) * channels + ch) * plane + e, masked, u8, out);
        }
      }
    }
  }
}

// ---- mu-fidelity's superpixel masks, one workgroup per mask: v = grid[m, cell[p]] * img[c, p], the min /
// max reduction over the mask's image, a barrier, then the outputs on a second evaluation (img, cell
// and the grid row come from L2 then). A cell outside [0, grid_len) multiplies by 0.
__device__ __forceinline__ float cell_value(const float* __restrict__ g, int32_t cell, int64_t grid_len) {
  return ((uint64_t)(int64_t)cell < (uint64_t)grid_len) ? g[cell] : 0.f;
}

template <int W>
__global__ void __launch_bounds__(1024) k_cell_mask_pixels(int channels, int64_t plane, const float* __restrict__ img,
                                                           int64_t grid_len, const float* __restrict__ grid,
                                                           const int32_t* __restrict__ cell, ChanNorm cn,
                                                           float* __restrict__ masked, uint8_t* __restrict__ u8,
                                                           float* __restrict__ out) {
  __shared__ float lut[4][256];
  __shared__ MinMax<float> red[16];
  if (out) fill_norm_lut(lut, channels, cn);
  const int64_t m = blockIdx.x;
  const float* g = grid + m * grid_len;
  const int64_t units = plane / W;
  float mn = INFINITY, mx = -INFINITY;
  for (int pass = 0; pass < 2; ++pass) {
    for (int64_t u = threadIdx.x; u < units; u += blockDim.x) {
      const int64_t e = u * W;
      float k[W];
      if constexpr (W == 4) {
        const int4 t = *reinterpret_cast<const int4*>(cell + e);
        k[0] = cell_value(g, t.x, grid_len), k[1] = cell_value(g, t.y, grid_len);
        k[2] = cell_value(g, t.z, grid_len), k[3] = cell_value(g, t.w, grid_len);
      } else {
        k[0] = cell_value(g, cell[e], grid_len);
      }
      for (int ch = 0; ch < channels; ++ch) {
        float v[W];
        if constexpr (W == 4) {
          const wam_f4v t = *reinterpret_cast<const wam_f4v*>(img + ch * plane + e);
          v[0] = k[0] * t.x, v[1] = k[1] * t.y, v[2] = k[2] * t.z, v[3] = k[3] * t.w;
        } else {
          v[0] = k[0] * img[ch * plane + e];
        }
        if (pass == 0) {
#pragma unroll
          for (int i = 0; i < W; ++i) {
            mn = fminf(mn, v[i]);
            mx = fmaxf(mx, v[i]);
          }
        } else {
          emit<W>(v, mn, mx, lut[ch], (m * channels + ch) * plane + e, masked, u8, out);
        }
      }
    }
    if (pass == 0) {
      const MinMax<float> ext = block_reduce(MinMax<float>{mn, mx}, MinMaxOp(), red);
      mn = ext.mn, mx = ext.mx;
    }
  }
}

// ---- Grad-CAM / Grad-CAM++ of one image per workgroup, in float64 (the reference sums K float32
// planes one by one; float64 keeps the device within rounding of a float64 restatement whatever the
// order): channel weights (one wave per channel), the weighted sum over channels (the pixels times as
// many channel slices as the block holds, reduced through LDS in slice order), ReLU, - min, / max, and
// torch's bilinear resize (align_corners=False: float32 source coordinates, clamped at 0).
__global__ void __launch_bounds__(1024) k_cam_maps(int K, int h, int w, const float* __restrict__ act,
                                                   const float* __restrict__ grad, int plus_plus, int out_h,
                                                   int out_w, float* __restrict__ out) {
  extern __shared__ double cam_lds[];
  const int hw = h * w;
  double* wk = cam_lds;          // [K] channel weights
  double* cam = wk + K;          // [hw]
  double* part = cam + hw;       // [blockDim] partial sums of the channel slices
  double* red = part + blockDim.x;  // [16]
  const float* a = act + (int64_t)blockIdx.x * K * hw;
  const float* g = grad + (int64_t)blockIdx.x * K * hw;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  // a wave takes kCamGroup channels at a time, so that as many loads are in flight; each channel's sum
  // keeps its own order
  for (int k0 = wave * kCamGroup; k0 < K; k0 += nw * kCamGroup) {
    double sg[kCamGroup], sa[kCamGroup];
#pragma unroll
    for (int u = 0; u < kCamGroup; ++u) sg[u] = sa[u] = 0.0;
    for (int p = lane; p < hw; p += 64) {
#pragma unroll
      for (int u = 0; u < kCamGroup; ++u) {
        if (k0 + u >= K) continue;
        const double gv = g[(int64_t)(k0 + u) * hw + p];
        if (plus_plus) {
          const double av = a[(int64_t)(k0 + u) * hw + p];
          sg[u] += (gv > 0.0 ? gv : 0.0) * av;
          sa[u] += av;
        } else {
          sg[u] += gv;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kCamGroup; ++u) {
      for (int s = 32; s > 0; s >>= 1) {
        sg[u] += __shfl_xor(sg[u], s, 64);
        sa[u] += __shfl_xor(sa[u], s, 64);
      }
      if (lane == 0 && k0 + u < K) wk[k0 + u] = plus_plus ? sg[u] / (sa[u] + 1e-8) : sg[u] / (double)hw;
    }
  }
  __syncthreads();
  if (hw <= (int)blockDim.x) {
    const int slices = blockDim.x / hw;
    const int p = threadIdx.x % hw, sl = threadIdx.x / hw;
    if (sl < slices) {
      double acc = 0.0;
#pragma unroll 8
      for (int k = sl; k < K; k += slices) acc += wk[k] * (double)a[(int64_t)k * hw + p];
      part[sl * hw + p] = acc;
    }
    __syncthreads();
    if ((int)threadIdx.x < hw) {
      double acc = part[threadIdx.x];
      for (int i = 1; i < slices; ++i) acc += part[i * hw + threadIdx.x];
      cam[threadIdx.x] = acc;
    }
  } else {
    for (int p = threadIdx.x; p < hw; p += blockDim.x) {
      double acc = 0.0;
#pragma unroll 8
      for (int k = 0; k < K; ++k) acc += wk[k] * (double)a[(int64_t)k * hw + p];
      cam[p] = acc;
    }
  }
  __syncthreads();
  double mn = INFINITY;
  for (int p = threadIdx.x; p < hw; p += blockDim.x) {  // every thread re-reads only what it wrote
    const double c = cam[p] < 0.0 ? 0.0 : cam[p];
    cam[p] = c;
    mn = fmin(mn, c);
  }
  mn = block_reduce(mn, MinOp(), red);
  double mx = -INFINITY;
  for (int p = threadIdx.x; p < hw; p += blockDim.x) {
    const double c = cam[p] - mn;
    cam[p] = c;
    mx = fmax(mx, c);
  }
  mx = block_reduce(mx, MaxOp(), red);
  for (int p = threadIdx.x; p < hw; p += blockDim.x) cam[p] = cam[p] / mx;  // 0 / 0 = NaN: the whole map
  __syncthreads();
  const float sh = (float)h / (float)out_h, sw = (float)w / (float)out_w;
  float* o = out + (int64_t)blockIdx.x * out_h * out_w;
  for (int t = threadIdx.x; t < out_h * out_w; t += blockDim.x) {
    const int oy = t / out_w, ox = t - oy * out_w;
    float fy = __fmul_rn(sh, (float)oy + 0.5f) - 0.5f, fx = __fmul_rn(sw, (float)ox + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < h - 1 ? y0 : h - 1;
    x0 = x0 < w - 1 ? x0 : w - 1;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
    ly1 = fminf(fmaxf(ly1, 0.f), 1.f);
    lx1 = fminf(fmaxf(lx1, 0.f), 1.f);
    const double ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const double top = lx0 * cam[y0 * w + x0] + (double)lx1 * cam[y0 * w + x1];
    const double bot = lx0 * cam[y1 * w + x0] + (double)lx1 * cam[y1 * w + x1];
    o[t] = (float)(ly0 * top + (double)ly1 * bot);
  }
}

// ---- the channel mean every gradient method ends in: numpy's float32 mean over a short axis
__global__ void __launch_bounds__(256) k_channel_mean(int64_t items, int channels, int64_t plane,
                                                      const float* __restrict__ g, const float* __restrict__ mult,
                                                      int absolute, float* __restrict__ out_f32,
                                                      double* __restrict__ acc_f64) {
  const int64_t total = items * plane;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = t / plane, p = t - n * plane;
    float sum = 0.f;
    for (int c = 0; c < channels; ++c) {
      const int64_t at = (n * channels + c) * plane + p;
      float v = g[at];
      if (mult) v = __fmul_rn(v, mult[at]);
      if (absolute) v = fabsf(v);
      sum = c ? __fadd_rn(sum, v) : v;
    }
    const float m = __fdiv_rn(sum, (float)channels);
    if (out_f32) out_f32[t] = m;
    if (acc_f64) acc_f64[t] += (double)m;
  }
}

}  // namespace

extern "C" {

int64_t wam_rank_mask_pixels_ws_bytes(int64_t sets, int64_t n_iter) {
  if (sets < 0 || n_iter < 1) return -1;
  return sets * (n_iter + 1 + (int64_t)kMaxSplits * (n_iter + 2)) * 2 * (int64_t)sizeof(float);
}

int wam_rank_mask_pixels(int64_t sets, int channels, int64_t plane, const float* img, const int32_t* rank,
                         int64_t n_iter, int64_t n_comp, int deletion, const float* mean, const float* std,
                         float* masked, uint8_t* u8, float* out, void* ws, void* stream) {
  if (sets < 0 || sets > 65535 || channels < 1 || channels > 4 || plane < 1 || plane > INT32_MAX || n_iter < 1 ||
      n_comp < 0 || n_comp > INT32_MAX || !img || !rank || !ws || (!masked && !u8 && !out) || (out && (!mean || !std)))
    return WAM_ERR_INVALID_ARG;
  if (n_iter > kMaxIter) return WAM_ERR_UNSUPPORTED;
  if (sets == 0) return WAM_OK;
  if (!aligned4(ws)) return WAM_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t M = n_iter + 1;
  float* ext = static_cast<float*>(ws);                                // [sets, M, 2]
  uint32_t* part = reinterpret_cast<uint32_t*>(ext + sets * M * 2);   // [sets, splits, 2, n_iter + 2]
  const int splits = (int)wam_grid(plane, 2048, kMaxSplits);
  {
    WamTimer tm(st, "k_rank_extrema", 4.0 * sets * (channels + 1) * plane + 8.0 * sets * splits * (n_iter + 2));
    hipLaunchKernelGGL(k_rank_extrema, dim3(splits, (unsigned)sets), dim3(256), 0, st, channels, plane, img, rank,
                       (int)n_iter, (int)n_comp, part);
    WAM_LAUNCH_CHECK();
  }
  {
    WamTimer tm(st, "k_rank_scan", 8.0 * sets * splits * (n_iter + 2) + 8.0 * sets * M);
    hipLaunchKernelGGL(k_rank_scan, dim3((unsigned)sets), dim3(256), 0, st, splits, (int)n_iter, deletion, part, ext);
    WAM_LAUNCH_CHECK();
  }
  const bool vec = (plane & 3) == 0 && aligned16(img) && aligned16(rank) && aligned16(masked) && aligned16(out) &&
                   aligned4(u8);
  const double px = (double)sets * M * channels * plane;
  WamTimer tm(st, "k_rank_mask_pixels", 4.0 * sets * (channels + 1) * plane + 8.0 * sets * M +
                                            px * ((masked ? 4.0 : 0.0) + (u8 ? 1.0 : 0.0) + (out ? 4.0 : 0.0)));
  const ChanNorm cn = chan_norm(channels, mean, std);
  const dim3 grid(wam_grid(vec ? plane >> 2 : plane, 256, 4096), (unsigned)((M + kMaskChunk - 1) / kMaskChunk),
                  (unsigned)sets);
  if (vec)
    hipLaunchKernelGGL(k_rank_mask_pixels<4>, grid, dim3(256), 0, st, sets, channels, plane, img, rank, n_iter, n_comp,
                       deletion, cn, ext, masked, u8, out);
  else
    hipLaunchKernelGGL(k_rank_mask_pixels<1>, grid, dim3(256), 0, st, sets, channels, plane, img, rank, n_iter, n_comp,
                       deletion, cn, ext, masked, u8, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int wam_cell_mask_pixels(int channels, int64_t plane, const float* img, int64_t n_masks, int64_t grid_len,
                         const float* grid, const int32_t* cell, const float* mean, const float* std, float* masked,
                         uint8_t* u8, float* out, void* stream) {
  if (channels < 1 || channels > 4 || plane < 1 || plane > INT32_MAX || n_masks < 0 || n_masks > INT32_MAX ||
      grid_len < 1 || !img || !grid || !cell || (!masked && !u8 && !out) || (out && (!mean || !std)))
    return WAM_ERR_INVALID_ARG;
  if (n_masks == 0) return WAM_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (plane & 3) == 0 && aligned16(img) && aligned16(cell) && aligned16(masked) && aligned16(out) &&
                   aligned4(u8);
  const double px = (double)n_masks * channels * plane;
  WamTimer tm(st, "k_cell_mask_pixels", 4.0 * (channels + 1) * plane + 4.0 * n_masks * grid_len +
                                            px * ((masked ? 4.0 : 0.0) + (u8 ? 1.0 : 0.0) + (out ? 4.0 : 0.0)));
  const ChanNorm cn = chan_norm(channels, mean, std);
  if (vec)
    hipLaunchKernelGGL(k_cell_mask_pixels<4>, dim3((unsigned)n_masks), dim3(1024), 0, st, channels, plane, img,
                       grid_len, grid, cell, cn, masked, u8, out);
  else
    hipLaunchKernelGGL(k_cell_mask_pixels<1>, dim3((unsigned)n_masks), dim3(1024), 0, st, channels, plane, img,
                       grid_len, grid, cell, cn, masked, u8, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int wam_cam_maps(int64_t images, int64_t K, int h, int w, const float* act, const float* grad, int plus_plus,
                 int out_h, int out_w, float* out, void* stream) {
  if (images < 0 || images > INT32_MAX || K < 1 || h < 1 || w < 1 || out_h < 1 || out_w < 1 || !act || !grad || !out)
    return WAM_ERR_INVALID_ARG;
  if ((int64_t)h * w > INT32_MAX || (int64_t)out_h * out_w > INT32_MAX) return WAM_ERR_INVALID_ARG;
  const int block = 1024;
  const int64_t lds = 8 * (K + (int64_t)h * w + block + 16);
  if (lds > kCamLdsCap) return WAM_ERR_UNSUPPORTED;
  if (images == 0) return WAM_OK;
  if (int rc = wam_lds_opt_in((const void*)k_cam_maps, kCamLdsCap)) return rc;
  hipStream_t st = (hipStream_t)stream;
  WamTimer tm(st, "k_cam_maps", 8.0 * images * K * h * w + 4.0 * images * out_h * out_w);
  hipLaunchKernelGGL(k_cam_maps, dim3((unsigned)images), dim3(block), (size_t)lds, st, (int)K, h, w, act, grad, plus_plus,
                     out_h, out_w, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int wam_channel_mean(int64_t items, int channels, int64_t plane, const float* g, const float* mult, int absolute,
                     float* out_f32, double* acc_f64, void* stream) {
  if (items < 0 || channels < 1 || plane < 1 || !g || (!out_f32 && !acc_f64)) return WAM_ERR_INVALID_ARG;
  const int64_t work = items * plane;
  if (work == 0) return WAM_OK;
  WamTimer tm((hipStream_t)stream, "k_channel_mean",
              4.0 * work * channels * (mult ? 2 : 1) + work * ((out_f32 ? 4.0 : 0.0) + (acc_f64 ? 16.0 : 0.0)));
  hipLaunchKernelGGL(k_channel_mean, dim3(wam_grid(work, 256)), dim3(256), 0, (hipStream_t)stream, items, channels, plane,
                     g, mult, absolute, out_f32, acc_f64);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

}  // extern "C"
