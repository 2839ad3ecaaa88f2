// Audio insertion / deletion / faithfulness of spectra / input fidelity (Eval1DWAM,
// src/evaluators.py:39-306): the ranking-to-masked-input path between wam_wavedec and wam_waverec,
// and the peak normalisation between wam_waverec and the mel front-end. Per clip the reference
// builds n_iter + 1 masks on the host, multiplies them into the coefficients band by band, runs a
// float64 pywt.waverec of every masked set and divides each reconstruction by its maximum in numpy.
// Here the masks are never stored: one pass turns the ranking into the masked band-major
// coefficients of every (clip, mask) item wam_waverec reads, and one workgroup per reconstruction
// does the max reduction and the division. All three kernels are HBM-bound streaming passes.
#include "quantize.hpp"
#include "rankmask.hpp"

namespace {

constexpr int kMaxBands1D = 1 + WAM_MAX_LEVELS;

// ---- out = in / max(in), one workgroup per row: wave-64 shuffles, one LDS step, 16-byte loads when
// the rows are 16-byte aligned; the second read of the row comes from L2.
__global__ void __launch_bounds__(1024) k_peak_normalize(int64_t len, const float* in, float* out,
                                                         int32_t* __restrict__ silent, int zero_silent, int vec) {
  const float* x = in + blockIdx.x * len;
  float* o = out + blockIdx.x * len;
  const int64_t n4 = len >> 2;
  float mx = -INFINITY;
  if (vec) {
    const wam_f4v* x4 = reinterpret_cast<const wam_f4v*>(x);
    for (int64_t i = threadIdx.x; i < n4; i += blockDim.x) {
      const wam_f4v v = x4[i];
      mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
  } else {
    for (int64_t i = threadIdx.x; i < len; i += blockDim.x) mx = fmaxf(mx, x[i]);
  }
  __shared__ float red[16];
  mx = block_reduce(mx, MaxOp(), red);
  const bool sil = mx == 0.f;
  if (threadIdx.x == 0 && silent) silent[blockIdx.x] = sil ? 1 : 0;
  if (sil && zero_silent) {
    if (o == x) return;
    for (int64_t i = threadIdx.x; i < len; i += blockDim.x) o[i] = x[i];
    return;
  }
  // every element is read and then written by the same thread: in place is safe
  if (vec) {
    const wam_f4v* x4 = reinterpret_cast<const wam_f4v*>(x);
    wam_f4v* o4 = reinterpret_cast<wam_f4v*>(o);
    for (int64_t i = threadIdx.x; i < n4; i += blockDim.x) {
      wam_f4v v = x4[i];
      v.x = __fdiv_rn(v.x, mx);
      v.y = __fdiv_rn(v.y, mx);
      v.z = __fdiv_rn(v.z, mx);
      v.w = __fdiv_rn(v.w, mx);
      o4[i] = v;
    }
  } else {
    for (int64_t i = threadIdx.x; i < len; i += blockDim.x) o[i] = __fdiv_rn(x[i], mx);
  }
}

// the first half of k_peak_normalize alone (route 0's row maxima): one workgroup per row, a zero
// maximum written as +0.0f
__global__ void __launch_bounds__(1024) k_row_max(int64_t len, const float* __restrict__ in,
                                                  float* __restrict__ row_max, int vec) {
  const float* x = in + blockIdx.x * len;
  float mx = -INFINITY;
  if (vec) {
    const wam_f4v* x4 = reinterpret_cast<const wam_f4v*>(x);
    for (int64_t i = threadIdx.x; i < (len >> 2); i += blockDim.x) {
      const wam_f4v v = x4[i];
      mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
  } else {
    for (int64_t i = threadIdx.x; i < len; i += blockDim.x) mx = fmaxf(mx, x[i]);
  }
  __shared__ float red[16];
  mx = block_reduce(mx, MaxOp(), red);
  if (threadIdx.x == 0) row_max[blockIdx.x] = mx == 0.f ? 0.f : mx;
}

// ---- out = in / row_max, the second half of k_peak_normalize with the maxima given: a workgroup takes
// kDivSpan consecutive elements of one row, so every row is read once and written once by the whole chip
constexpr int kDivSpan = 256 * 16;

__global__ void __launch_bounds__(256) k_peak_divide(int64_t len, int64_t spans, const float* in,
                                                     const float* __restrict__ row_max, float* out,
                                                     int32_t* __restrict__ silent, int zero_silent, int vec) {
  const int64_t row = blockIdx.x / spans, sp = blockIdx.x - row * spans;
  const float mx = row_max[row];
  const bool sil = mx == 0.f;
  if (sp == 0 && threadIdx.x == 0 && silent) silent[row] = sil ? 1 : 0;
  const float* x = in + row * len;
  float* o = out + row * len;
  const int64_t i0 = sp * kDivSpan, i1 = i0 + kDivSpan < len ? i0 + kDivSpan : len;
  if (sil && zero_silent) {
    if (o == x) return;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) o[i] = x[i];
    return;
  }
  // every element is read and then written by the same thread: in place is safe
  if (vec) {
    const wam_f4v* x4 = reinterpret_cast<const wam_f4v*>(x);
    wam_f4v* o4 = reinterpret_cast<wam_f4v*>(o);
    for (int64_t i = (i0 >> 2) + threadIdx.x; i < (i1 >> 2); i += 256) {
      wam_f4v v = x4[i];
      v.x = __fdiv_rn(v.x, mx);
      v.y = __fdiv_rn(v.y, mx);
      v.z = __fdiv_rn(v.z, mx);
      v.w = __fdiv_rn(v.w, mx);
      o4[i] = v;
    }
  } else {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) o[i] = __fdiv_rn(x[i], mx);
  }
}

}  // namespace

// wam_waverec1_ranked's route 0 (evaluate_ranked.hip): the signed maximum of each of `rows` rows of `in`
int launch_row_max(int64_t rows, int64_t len, const float* in, float* row_max, hipStream_t st) {
  const int vec = (len & 3) == 0 && aligned16(in);
  WamTimer tm(st, "k_row_max", 4.0 * rows * len);
  hipLaunchKernelGGL(k_row_max, dim3((unsigned)rows), dim3(len >= 16384 ? 1024 : 256), 0, st, len, in, row_max, vec);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

extern "C" {

int wam_rank_mask_coeffs(const wam_plan* plan, int64_t sets, const float* coeffs, const int32_t* rank,
                         int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion,
                         float* out, void* stream) {
  if (!plan || sets < 0 || rank_len < 1 || n_iter < 1 || n_comp < 0 || !coeffs || !rank || !pos || !out)
    return WAM_ERR_INVALID_ARG;
  if (plan->ndim != 1 || plan->nbands > kMaxBands1D) return WAM_ERR_UNSUPPORTED;
  if (rank_len > INT32_MAX) return WAM_ERR_INVALID_ARG;
  const bool ptrs_aligned = aligned16(coeffs) && aligned16(pos) && aligned16(out);
  return launch_rank_mask<kMaxBands1D>(false, sets, 1, plan->nbands, plan->band_off, ptrs_aligned, coeffs, rank,
                                       rank_len, pos, n_iter, n_comp, deletion, out, (hipStream_t)stream,
                                       "k_rank_mask_coeffs");
}

int wam_rank_mask_rows(int64_t sets, int64_t len, const float* src, const int32_t* rank, int64_t n_iter,
                       int64_t n_comp, int deletion, float* out, void* stream) {
  if (sets < 0 || len < 1 || len > INT32_MAX || n_iter < 1 || n_comp < 0 || !src || !rank || !out)
    return WAM_ERR_INVALID_ARG;
  const int64_t band_off[2] = {0, len};
  return launch_rank_mask<kMaxBands1D>(true, sets, 1, 1, band_off, aligned16(src) && aligned16(rank) && aligned16(out),
                                       src, rank, len, nullptr, n_iter, n_comp, deletion, out, (hipStream_t)stream,
                                       "k_rank_mask_rows");
}

int wam_peak_normalize(int64_t rows, int64_t len, const float* in, float* out, int32_t* silent, int zero_silent,
                       void* stream) {
  if (rows < 0 || rows > INT32_MAX || len < 1 || !in || !out) return WAM_ERR_INVALID_ARG;
  if (rows == 0) return WAM_OK;
  const int vec = (len & 3) == 0 && aligned16(in) && aligned16(out);
  WamTimer tm((hipStream_t)stream, "k_peak_normalize", 8.0 * rows * len);
  hipLaunchKernelGGL(k_peak_normalize, dim3((unsigned)rows), dim3(len >= 16384 ? 1024 : 256), 0, (hipStream_t)stream,
                     len, in, out, silent, zero_silent, vec);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int wam_peak_divide(int64_t rows, int64_t len, const float* in, const float* row_max, float* out, int32_t* silent,
                    int zero_silent, void* stream) {
  if (rows < 0 || rows > INT32_MAX || len < 1 || !in || !row_max || !out) return WAM_ERR_INVALID_ARG;
  if (rows == 0) return WAM_OK;
  const int64_t spans = (len + kDivSpan - 1) / kDivSpan;
  if (rows * spans > INT32_MAX) return WAM_ERR_INVALID_ARG;
  const int vec = (len & 3) == 0 && aligned16(in) && aligned16(out);
  WamTimer tm((hipStream_t)stream, "k_peak_divide", 8.0 * rows * len);
  hipLaunchKernelGGL(k_peak_divide, dim3((unsigned)(rows * spans)), dim3(256), 0, (hipStream_t)stream, len, spans, in,
                     row_max, out, silent, zero_silent, vec);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

}  // extern "C"
