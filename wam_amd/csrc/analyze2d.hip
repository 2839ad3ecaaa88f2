// WAMAnalyzer2D (src/analyzers.py:16-203, helpers src/analyzers_helpers.py:6-134): which coefficients
// the model needs (isolate_necessary_components: quantile thresholds on the WAM map) and what each
// scale contributes (isolate_scales: one mask per level). Per image and per quantile the reference
// runs pywt.wavedec2 -> coeffs_to_array -> arr * (grad_wam >= t) -> waverec2 per channel on the CPU,
// then its own quantisation ((x - mn) / mx - mn) * 255 -> uint8 (wrapping) -> PIL -> transform. Here the
// analysis runs once for all images, one pass turns the thresholds into the masked band-major
// coefficients of every (image, threshold, channel) plane wam_waverec reads -- the masks are never
// stored -- and one workgroup per reconstruction does the min / max reduction and the quantisation.
// Both kernels are HBM-bound streaming passes.
#include "maskexpand.hpp"
#include "quantize.hpp"

namespace {

using ThrBands = MaskBands<WAM_MAX_BANDS>;

struct LevelEdges {
  int n;                            // entries (levels + 1)
  int e[WAM_MAX_LEVELS + 1];        // int(size / 2^j), j = 0 .. levels
};

// the map value at array position p of an image; a position outside the map is kept by no threshold
__device__ __forceinline__ double map_value(const double* __restrict__ w, int32_t p, int64_t map_len) {
  return ((uint64_t)(int64_t)p < (uint64_t)map_len) ? w[p] : (double)NAN;
}

// compute_levelized_masks: entry q < levels holds the three blocks [s:e, s:e], [s:e, :s], [:s, s:e] with
// s = e[q + 1], e = e[q], i.e. s <= max(row, col) < e; entry `levels` holds [:a, :a], a = e[levels].
// The table is read with constant indices only (it lives in the kernel arguments: a runtime index
// would copy it to scratch).
__device__ __forceinline__ void level_bounds(const LevelEdges& le, int q, int& lo, int& hi) {
  lo = 0;
  hi = 0;
  const int qe = q + 1 < le.n ? q : le.n - 1;       // the entry's outer edge
#pragma unroll
  for (int j = 0; j <= WAM_MAX_LEVELS; ++j) {
    if (j == qe) hi = le.e[j];
    if (j == q + 1 && q + 1 < le.n) lo = le.e[j];
  }
}

__device__ __forceinline__ bool in_level(int lo, int hi, int32_t p, int size) {
  const int r = p / size, c = p - r * size;
  const int m = r > c ? r : c;
  return m >= lo && m < hi;
}

__device__ __forceinline__ float keep_mul(double v, double t, bool strict) {
  return (strict ? v > t : v >= t) ? 1.f : 0.f;
}

// mask_expand's policy: an element's fate is the map value of its image at its array position; the
// "masks" are the thresholds of the image's row, the output item of (plane (n, c), threshold q) is
// (n * n_thr + q) * channels + c. LEVEL: threshold q is level entry q, a map value outside the entry's
// region counts as 0.
template <bool LEVEL>
struct ThresholdPolicy {
  int channels;
  const int32_t* __restrict__ pos;
  int size;
  int64_t map_len;
  const double* __restrict__ wam;
  int64_t n_thr;
  const double* __restrict__ thr;
  int64_t thr_stride;
  const LevelEdges& le;
  bool strict;
  struct Item { int64_t n, c; const double *w, *t; };  // image, channel, the image's map and threshold rows
  struct Elem { int32_t p; double v; };                // array position, map value there
  struct Mask { double t; int lo, hi; };               // threshold, the level entry's bounds
  __device__ Item item(int64_t pl) const {
    const int64_t n = pl / channels;
    return {n, pl - n * channels, wam + n * map_len, thr + n * thr_stride};
  }
  template <int W>
  __device__ void load(const Item& it, int64_t bo, int64_t e, Elem (&el)[W]) const {
    int32_t p[W];
    load_w<W>(pos + bo + e, p);
#pragma unroll
    for (int k = 0; k < W; ++k) el[k] = {p[k], map_value(it.w, p[k], map_len)};
  }
  __device__ Mask mask(const Item& it, int64_t q) const {
    Mask mk{it.t[q], 0, 0};
    if (LEVEL) level_bounds(le, (int)q, mk.lo, mk.hi);
    return mk;
  }
  __device__ float keep(const Mask& mk, const Elem& el) const {
    double v = el.v;
    if (LEVEL && (uint64_t)(int64_t)el.p < (uint64_t)map_len && !in_level(mk.lo, mk.hi, el.p, size)) v = 0.0;
    return keep_mul(v, mk.t, strict);
  }
  __device__ int64_t out_item(const Item& it) const { return it.n * n_thr * channels + it.c; }
  __device__ int64_t out_step() const { return channels; }
};

template <bool LEVEL>
__global__ void __launch_bounds__(256) k_threshold_mask(int64_t images, int channels, ThrBands tb,
                                                        const float* __restrict__ coeffs,
                                                        const int32_t* __restrict__ pos, int size,
                                                        const double* __restrict__ wam, int64_t n_thr,
                                                        const double* __restrict__ thr, int64_t thr_stride,
                                                        LevelEdges le, int strict, float* __restrict__ out) {
  const ThresholdPolicy<LEVEL> p{channels, pos, size, (int64_t)size * size, wam, n_thr, thr,
                                 thr_stride, le, strict != 0};
  mask_expand(p, tb, images * channels, n_thr, coeffs, out, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
              (int64_t)gridDim.x * blockDim.x);
}

// ---- quantisation of a reconstruction, one workgroup per image (channels x plane floats): the min / max
// pass (block_reduce), a barrier, then the map (quantize_one, quantize.hpp) on a second read of the image

// VEC: plane is a multiple of 4 and the buffers are 16-byte (u8: 4-byte) aligned, so a thread handles 4
// consecutive values of one channel per step: a 16-byte load, a 4-byte and a 16-byte store. The values are
// those of the scalar path (the same operations per element; the min / max do not depend on the order).
template <int RULE, bool VEC>
__global__ void __launch_bounds__(1024) k_quantize_ex(int channels, int64_t plane, const float* __restrict__ rec,
                                                      ChanNorm cn, uint8_t* __restrict__ u8,
                                                      float* __restrict__ out) {
  const int64_t n = (int64_t)channels * plane;
  const float* x = rec + blockIdx.x * n;
  float mn = INFINITY, mx = -INFINITY;
  if (VEC) {
    const wam_f4v* x4 = reinterpret_cast<const wam_f4v*>(x);
    for (int64_t i = threadIdx.x; i < (n >> 2); i += blockDim.x) {
      const wam_f4v v = x4[i];
      mn = fminf(fminf(mn, fminf(v.x, v.y)), fminf(v.z, v.w));
      mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
  } else {
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      mn = fminf(mn, x[i]);
      mx = fmaxf(mx, x[i]);
    }
  }
  __shared__ MinMax<float> red[16];
  const MinMax<float> ext = block_reduce(MinMax<float>{mn, mx}, MinMaxOp(), red);
  mn = ext.mn, mx = ext.mx;
  uint8_t* b = u8 ? u8 + blockIdx.x * n : nullptr;
  float* o = out ? out + blockIdx.x * n : nullptr;
  if (VEC) {
    const wam_f4v* x4 = reinterpret_cast<const wam_f4v*>(x);
    for (int64_t i = threadIdx.x; i < (n >> 2); i += blockDim.x) {
      const wam_f4v v = x4[i];
      const uint8_t q0 = quantize_one<RULE>(v.x, mn, mx), q1 = quantize_one<RULE>(v.y, mn, mx);
      const uint8_t q2 = quantize_one<RULE>(v.z, mn, mx), q3 = quantize_one<RULE>(v.w, mn, mx);
      if (b) reinterpret_cast<uchar4*>(b)[i] = make_uchar4(q0, q1, q2, q3);
      if (o) {
        const int c = (int)((i << 2) / plane);
        const float m = cn.mean[c], sd = cn.std[c];
        reinterpret_cast<wam_f4v*>(o)[i] =
            wam_f4v{__fdiv_rn(__fdiv_rn((float)q0, 255.f) - m, sd), __fdiv_rn(__fdiv_rn((float)q1, 255.f) - m, sd),
                    __fdiv_rn(__fdiv_rn((float)q2, 255.f) - m, sd), __fdiv_rn(__fdiv_rn((float)q3, 255.f) - m, sd)};
      }
    }
    return;
  }
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const uint8_t q = quantize_one<RULE>(x[i], mn, mx);
    if (b) b[i] = q;
    if (o) {
      const int c = (int)(i / plane);
      o[i] = __fdiv_rn(__fdiv_rn((float)q, 255.f) - cn.mean[c], cn.std[c]);
    }
  }
}

template <int RULE, bool VEC>
void launch_quantize_as(int64_t images, int channels, int64_t plane, const float* rec, const ChanNorm& cn, uint8_t* u8,
                        float* out, hipStream_t st) {
  hipLaunchKernelGGL((k_quantize_ex<RULE, VEC>), dim3((unsigned)images), dim3(1024), 0, st, channels, plane, rec, cn, u8,
                     out);
}

int launch_quantize(int64_t images, int channels, int64_t plane, const float* rec, int rule, const float* mean,
                    const float* std, uint8_t* u8, float* out, hipStream_t st) {
  const ChanNorm cn = chan_norm(channels, mean, std);
  const double px = (double)images * channels * plane;
  const char* name = rule ? "k_quantize_analyzer" : (out ? "k_quantize_normalize" : "k_quantize_u8");
  const bool vec = (plane & 3) == 0 && aligned16(rec) && (!out || aligned16(out)) && aligned4(u8);
  WamTimer tm(st, name, px * (4.0 + (u8 ? 1.0 : 0.0) + (out ? 4.0 : 0.0)));
  if (rule) {
    if (vec) launch_quantize_as<1, true>(images, channels, plane, rec, cn, u8, out, st);
    else launch_quantize_as<1, false>(images, channels, plane, rec, cn, u8, out, st);
  } else {
    if (vec) launch_quantize_as<0, true>(images, channels, plane, rec, cn, u8, out, st);
    else launch_quantize_as<0, false>(images, channels, plane, rec, cn, u8, out, st);
  }
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

}  // namespace

extern "C" {

int wam_threshold_mask_coeffs(const wam_plan* plan, int64_t images, int channels, const float* coeffs,
                              const int32_t* pos, int size, const double* wam, int64_t n_thr, const double* thr,
                              int64_t thr_stride, int level_mode, const int32_t* edges, int strict, float* out,
                              void* stream) {
  if (!plan || images <= 0 || n_thr <= 0 || channels < 1 || size < 1 || thr_stride < n_thr || !coeffs || !pos ||
      !wam || !thr || !out)
    return WAM_ERR_INVALID_ARG;
  if (plan->ndim != 2) return WAM_ERR_UNSUPPORTED;
  if ((int64_t)size * size > INT32_MAX) return WAM_ERR_INVALID_ARG;
  LevelEdges le{};
  if (level_mode) {
    if (!edges || n_thr > WAM_MAX_LEVELS + 1) return WAM_ERR_INVALID_ARG;
    le.n = (int)n_thr;
    for (int j = 0; j < le.n; ++j) le.e[j] = edges[j];
  }
  const int64_t planes = images * channels;
  ThrBands tb{};
  const int64_t units = fill_mask_bands(tb, plan->nbands, plan->band_off, planes,
                                        aligned16(coeffs) && aligned16(pos) && aligned16(out));
  if (units == 0) return WAM_OK;
  const int64_t K = tb.off[tb.nbands];
  const int64_t chunks = (n_thr + kMaskChunk - 1) / kMaskChunk;
  if (chunks > 65535) return WAM_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  // every input read once (the map at the K positions of each image), every output written once
  WamTimer tm(st, "k_threshold_mask", 4.0 * planes * K + 4.0 * K + 8.0 * images * K + 8.0 * images * n_thr +
                                          4.0 * (double)planes * n_thr * K);
  const dim3 grid(wam_grid(units, 256), (unsigned)chunks);
  if (level_mode)
    hipLaunchKernelGGL(k_threshold_mask<true>, grid, dim3(256), 0, st, images, channels, tb, coeffs, pos, size, wam,
                       n_thr, thr, thr_stride, le, strict, out);
  else
    hipLaunchKernelGGL(k_threshold_mask<false>, grid, dim3(256), 0, st, images, channels, tb, coeffs, pos, size, wam,
                       n_thr, thr, thr_stride, le, strict, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int wam_quantize_normalize_ex(int64_t images, int channels, int64_t plane, const float* rec, int rule,
                              const float* mean, const float* std, uint8_t* u8, float* out, void* stream) {
  if (images < 0 || images > INT32_MAX || channels < 1 || channels > 4 || plane < 1 || !rec || (rule != 0 && rule != 1) ||
      (!u8 && !out) || (out && (!mean || !std)))
    return WAM_ERR_INVALID_ARG;
  if (images == 0) return WAM_OK;
  return launch_quantize(images, channels, plane, rec, rule, mean, std, u8, out, (hipStream_t)stream);
}

int wam_quantize_resize_normalize_ex(int64_t images, int channels, int in_h, int in_w, const float* rec, int rule,
                                     int out_h, int out_w, int ksize_h, const int32_t* bounds_h, const int32_t* kk_h,
                                     int ksize_v, const int32_t* bounds_v, const int32_t* kk_v, int y0, int tmp_h,
                                     const float* mean, const float* std, uint8_t* scratch, float* out,
                                     void* stream) {
  if (images < 0 || images > INT32_MAX || channels < 1 || channels > 4 || in_h < 1 || in_w < 1 || out_h < 1 ||
      out_w < 1 || !rec || (rule != 0 && rule != 1) || !mean || !std || !scratch || !out)
    return WAM_ERR_INVALID_ARG;
  const bool horiz = bounds_h != nullptr, vert = bounds_v != nullptr;
  if ((horiz && (!kk_h || ksize_h < 1)) || (vert && (!kk_v || ksize_v < 1))) return WAM_ERR_INVALID_ARG;
  if (!horiz && out_w != in_w) return WAM_ERR_SHAPE;
  if (!vert && out_h != in_h) return WAM_ERR_SHAPE;
  if (horiz && (y0 < 0 || tmp_h < 1 || y0 + tmp_h > in_h)) return WAM_ERR_SHAPE;
  if (images == 0) return WAM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_quantize(images, channels, (int64_t)in_h * in_w, rec, rule, nullptr, nullptr, scratch, nullptr, st);
  if (rc != WAM_OK) return rc;
  return launch_pil_resize_norm(images, channels, in_h, in_w, out_h, out_w, ksize_h, bounds_h, kk_h, ksize_v, bounds_v,
                                kk_v, y0, tmp_h, mean, std, scratch, out, st);
}

}  // extern "C"
