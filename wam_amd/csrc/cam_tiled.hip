// Grad-CAM / Grad-CAM++ for target layers whose map does not fit one workgroup's LDS (k_cam_maps of
// baselines2d.hip holds the whole plane and all K weights there: K + h * w <= 19,440). Audio CNNs keep
// the full mel resolution through their first blocks (157 x 128 cells at the c3 shape, 431 x 128 at the
// reference's ESC-50 shape), and so does layer1 of an image ResNet from 640^2 inputs up. Same contract,
// same float64 arithmetic, three launches in stream order with the plane in a workspace (it is read back
// from L2 by the resize):
//   k_cam_weight_parts  a wave per (image, channel, split of the plane): float64 partial sums to ws
//   k_cam_plane         a workgroup per (1024-pixel tile, image): the partials combined split by split,
//                       k ascending in float64, ReLU, the plane and the tile's extrema to ws
//   k_cam_resize        each workgroup folds its image's tile extrema, then writes output pixels with
//                       the four-tap formula of k_cam_maps
// No floating-point atomics: every sum has one fixed order, two calls return the same bits. A lane (a
// thread) owns the same pixels in the same order on the 16-byte and on the scalar load path, so the
// values do not depend on the path either.
#include "maskexpand.hpp"
#include "quantize.hpp"

namespace {

constexpr int kCamTile = 1024;      // pixels of a k_cam_plane workgroup: 256 threads x 4
constexpr int kCamSeg = 1024;       // pixels a wave sums per split, until kCamMaxSplits is reached
constexpr int kCamMaxSplits = 64;
constexpr int kCamChunk = 256;      // channel weights a k_cam_plane workgroup holds in LDS at a time

inline int cam_splits(int64_t hw) {
  const int64_t s = (hw + kCamSeg - 1) / kCamSeg;
  return (int)(s < kCamMaxSplits ? s : kCamMaxSplits);
}
inline int64_t cam_tiles(int64_t hw) { return (hw + kCamTile - 1) / kCamTile; }

// four consecutive floats from p[0 .. n): one 16-byte load (VEC: n == 4 and p is 16-byte aligned) or
// up to four scalar ones
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t n, float* v) {
  if constexpr (VEC) {
    const wam_f4v t = *reinterpret_cast<const wam_f4v*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < n ? p[j] : 0.f;
  }
}

// ---- launch 1. Unit u = (image * K + k) * S + split is one wave: lane l adds the pixels
// seg0 + (it * 64 + l) * 4 + j in (it, j) order, the lanes meet in a xor butterfly. part [images, K, S, 2]
// = (sum grad | sum max(grad, 0) * act, sum act). max(grad, 0) * act is exact in float64.
template <bool VEC>
__global__ void __launch_bounds__(256) k_cam_weight_parts(int64_t units, int S, int64_t hw, int64_t seg,
                                                          const float* __restrict__ act,
                                                          const float* __restrict__ grad, int plus_plus,
                                                          double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= units) return;
  const int64_t ck = u / S, split = u - ck * S;
  const int64_t p0 = split * seg, p1 = p0 + seg < hw ? p0 + seg : hw;
  const float* g = grad + ck * hw;
  const float* a = act + ck * hw;
  double sg = 0.0, sa = 0.0;
#pragma unroll 2
  for (int64_t p = p0 + lane * 4; p < p1; p += 256) {
    float gv[4], av[4];
    load4<VEC>(g + p, p1 - p, gv);
    if (plus_plus) {
      load4<VEC>(a + p, p1 - p, av);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sg += (double)(gv[j] > 0.f ? gv[j] : 0.f) * (double)av[j];
        sa += (double)av[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) sg += (double)gv[j];
    }
  }
  for (int s = 32; s > 0; s >>= 1) {
    sg += __shfl_xor(sg, s, 64);
    sa += __shfl_xor(sa, s, 64);
  }
  if (lane == 0) {
    part[u * 2] = sg;
    part[u * 2 + 1] = sa;
  }
}

// ---- launch 2. Thread t of tile b owns the pixels b * 1024 + 4 t + j (W == 4: one 16-byte load per
// channel) or b * 1024 + 256 j + t (W == 1: coalesced scalar loads), j = 0 .. 3. The weights of
// kCamChunk channels at a time are combined from the partials (split order) into LDS; K is not bounded.
template <int W>
__global__ void __launch_bounds__(256) k_cam_plane(int64_t images, int64_t K, int S, int64_t hw,
                                                   const float* __restrict__ act, const double* __restrict__ part,
                                                   int plus_plus, double* __restrict__ plane,
                                                   double* __restrict__ ext) {
  __shared__ double wk[kCamChunk];
  __shared__ MinMax<double> red[4];
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * kCamTile;
  int64_t px[4];
  bool in[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    px[j] = W == 4 ? q0 + 4 * t + j : q0 + 256 * j + t;
    in[j] = px[j] < hw;
  }
  for (int64_t n = blockIdx.y; n < images; n += gridDim.y) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = 0; k0 < K; k0 += kCamChunk) {
      __syncthreads();  // the previous chunk's weights are still being read
      if (k0 + t < K) {
        const double* pp = part + ((n * K + k0 + t) * S) * 2;
        double sg = 0.0, sa = 0.0;
        for (int s = 0; s < S; ++s) {
          sg += pp[2 * s];
          sa += pp[2 * s + 1];
        }
        wk[t] = plus_plus ? sg / (sa + 1e-8) : sg / (double)hw;
      }
      __syncthreads();
      const int kn = (int)(K - k0 < kCamChunk ? K - k0 : kCamChunk);
      const float* a = act + (n * K + k0) * hw;
#pragma unroll 4
      for (int k = 0; k < kn; ++k, a += hw) {
        const double wv = wk[k];
        if constexpr (W == 4) {
          if (in[0]) {  // hw % 4 == 0: the four pixels are inside together
            const wam_f4v v = *reinterpret_cast<const wam_f4v*>(a + px[0]);
            acc[0] = fma(wv, (double)v.x, acc[0]);
            acc[1] = fma(wv, (double)v.y, acc[1]);
            acc[2] = fma(wv, (double)v.z, acc[2]);
            acc[3] = fma(wv, (double)v.w, acc[3]);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (in[j]) acc[j] = fma(wv, (double)a[px[j]], acc[j]);
        }
      }
    }
    MinMax<double> mm{INFINITY, -INFINITY};
    double* o = plane + n * hw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!in[j]) continue;
      const double c = acc[j] < 0.0 ? 0.0 : acc[j];
      o[px[j]] = c;
      mm.mn = fmin(mm.mn, c);
      mm.mx = fmax(mm.mx, c);
    }
    mm = block_reduce(mm, MinMaxOp(), red);
    if (t == 0) {
      double* e = ext + (n * gridDim.x + blockIdx.x) * 2;
      e[0] = mm.mn;
      e[1] = mm.mx;
    }
  }
}

// ---- launch 3. min and max of the ReLU'd plane from the tile extrema (minimum and maximum are exact: any
// order), max(cam - mn) = fl(max(cam) - mn) because rounding is monotone; then k_cam_maps' resize, every
// tap normalised as it is read: (cam - mn) / mx, 0 / 0 = NaN for the whole map.
__global__ void __launch_bounds__(256) k_cam_resize(int64_t images, int h, int w, int64_t tiles,
                                                    const double* __restrict__ plane, const double* __restrict__ ext,
                                                    int out_h, int out_w, float* __restrict__ out) {
  __shared__ MinMax<double> red[4];
  const int64_t hw = (int64_t)h * w, out_px = (int64_t)out_h * out_w;
  const float sh = (float)h / (float)out_h, sw = (float)w / (float)out_w;
  for (int64_t n = blockIdx.y; n < images; n += gridDim.y) {
    MinMax<double> mm{INFINITY, -INFINITY};
    const double* e = ext + n * tiles * 2;
    for (int64_t i = threadIdx.x; i < tiles; i += blockDim.x) {
      mm.mn = fmin(mm.mn, e[2 * i]);
      mm.mx = fmax(mm.mx, e[2 * i + 1]);
    }
    mm = block_reduce(mm, MinMaxOp(), red);
    const double mn = mm.mn, mx = mm.mx - mm.mn;
    const double* cam = plane + n * hw;
    float* o = out + n * out_px;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < out_px; t += (int64_t)gridDim.x * blockDim.x) {
      const int oy = (int)(t / out_w), ox = (int)(t - (int64_t)oy * out_w);
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
      const int64_t r0 = (int64_t)y0 * w, r1 = (int64_t)y1 * w;
      const double c00 = (cam[r0 + x0] - mn) / mx, c01 = (cam[r0 + x1] - mn) / mx;
      const double c10 = (cam[r1 + x0] - mn) / mx, c11 = (cam[r1 + x1] - mn) / mx;
      const double top = lx0 * c00 + (double)lx1 * c01;
      const double bot = lx0 * c10 + (double)lx1 * c11;
      o[t] = (float)(ly0 * top + (double)ly1 * bot);
    }
  }
}

}  // namespace

extern "C" {

int64_t wam_cam_maps_tiled_ws_bytes(int64_t images, int64_t K, int h, int w) {
  if (images < 0 || images > INT32_MAX || K < 1 || h < 1 || w < 1 || (int64_t)h * w > INT32_MAX) return -1;
  const int64_t hw = (int64_t)h * w;
  return 8 * images * (2 * K * cam_splits(hw) + hw + 2 * cam_tiles(hw));
}

int wam_cam_maps_tiled(int64_t images, int64_t K, int h, int w, const float* act, const float* grad, int plus_plus,
                       int out_h, int out_w, float* out, void* ws, int64_t ws_bytes, void* stream) {
  if (images < 0 || images > INT32_MAX || K < 1 || h < 1 || w < 1 || out_h < 1 || out_w < 1 || !act || !grad || !out)
    return WAM_ERR_INVALID_ARG;
  if ((int64_t)h * w > INT32_MAX || (int64_t)out_h * out_w > INT32_MAX) return WAM_ERR_INVALID_ARG;
  if (images == 0) return WAM_OK;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < wam_cam_maps_tiled_ws_bytes(images, K, h, w))
    return WAM_ERR_INVALID_ARG;
  const int64_t hw = (int64_t)h * w, tiles = cam_tiles(hw), out_px = (int64_t)out_h * out_w;
  const int S = cam_splits(hw);
  const int64_t seg = (((hw + S - 1) / S) + 3) & ~(int64_t)3;  // a multiple of 4: the 16-byte path splits nothing
  const int64_t units = images * K * S;
  if ((units + 3) / 4 > INT32_MAX) return WAM_ERR_UNSUPPORTED;
  double* part = static_cast<double*>(ws);   // [images, K, S, 2]
  double* plane = part + units * 2;          // [images, hw]
  double* ext = plane + images * hw;         // [images, tiles, 2]
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (hw & 3) == 0 && aligned16(act) && aligned16(grad);
  const unsigned gy = (unsigned)(images < 65535 ? images : 65535);
  {
    WamTimer tm(st, "k_cam_weight_parts", 4.0 * images * K * hw * (plus_plus ? 2 : 1) + 16.0 * units);
    const dim3 grid((unsigned)((units + 3) / 4));
    if (vec)
      hipLaunchKernelGGL(k_cam_weight_parts<true>, grid, dim3(256), 0, st, units, S, hw, seg, act, grad, plus_plus, part);
    else
      hipLaunchKernelGGL(k_cam_weight_parts<false>, grid, dim3(256), 0, st, units, S, hw, seg, act, grad, plus_plus, part);
    WAM_LAUNCH_CHECK();
  }
  {
    WamTimer tm(st, "k_cam_plane", 4.0 * images * K * hw + 16.0 * units + 8.0 * images * (hw + 2 * tiles));
    const dim3 grid((unsigned)tiles, gy);
    if (vec)
      hipLaunchKernelGGL(k_cam_plane<4>, grid, dim3(256), 0, st, images, K, S, hw, act, part, plus_plus, plane, ext);
    else
      hipLaunchKernelGGL(k_cam_plane<1>, grid, dim3(256), 0, st, images, K, S, hw, act, part, plus_plus, plane, ext);
    WAM_LAUNCH_CHECK();
  }
  WamTimer tm(st, "k_cam_resize", 8.0 * images * (hw + 2 * tiles) + 4.0 * images * out_px);
  hipLaunchKernelGGL(k_cam_resize, dim3(wam_grid(out_px, 256, 4096), gy), dim3(256), 0, st, images, h, w, tiles, plane,
                     ext, out_h, out_w, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

}  // extern "C"
