// Audio insertion / deletion / faithfulness of spectra / input fidelity (Eval1DWAM,
// src/evaluators.py:39-306): the ranking-to-masked-input path between wam_wavedec and wam_waverec,
// and the peak normalisation between wam_waverec and the mel front-end. Per clip the reference
// builds n_iter + 1 masks on the host, multiplies them into the coefficients band by band, runs a
// float64 pywt.waverec of every masked set and divides each reconstruction by its maximum in numpy.
// Here the masks are never stored: one pass turns the ranking into the masked band-major
// coefficients of every (clip, mask) item wam_waverec reads, and one workgroup per reconstruction
// does the max reduction and the division. All three kernels are HBM-bound streaming passes.
#include "maskexpand.hpp"
#include "quantize.hpp"

namespace {

constexpr int kMaxBands1D = 1 + WAM_MAX_LEVELS;
constexpr int kMaxBands3D = WAM_MAX_BANDS;  // 1 + 7 * levels: the expansion of wam_waverec_ranked's route 0

// mask_expand's policy: an element's fate is the rank of its mask slot pos[k] in its set's row.
// IDENT: the slot of element k is k (wam_rank_mask_rows), pos is not read.
template <bool IDENT>
struct RankPolicy {
  const int32_t* __restrict__ rank;
  int64_t rank_len;
  const int32_t* __restrict__ pos;
  int64_t n_iter, n_comp;
  bool del;
  struct Item { int64_t s; const int32_t* rk; };  // the set and its rank row
  using Elem = int32_t;
  using Mask = int64_t;
  __device__ Item item(int64_t s) const { return {s, rank + s * rank_len}; }
  template <int W>
  __device__ void load(const Item& it, int64_t bo, int64_t e, Elem (&rk)[W]) const {
    if (IDENT) return load_w<W>(it.rk + e, rk);
    int32_t p[W];
    load_w<W>(pos + bo + e, p);
#pragma unroll
    for (int k = 0; k < W; ++k) rk[k] = slot_rank(it.rk, p[k], rank_len);
  }
  __device__ Mask mask(const Item&, int64_t m) const { return mask_thr(m, n_iter, n_comp, rank_len); }
  __device__ float keep(Mask thr, Elem rk) const { return (((int64_t)rk < thr) != del) ? 1.f : 0.f; }
  __device__ int64_t out_item(const Item& it) const { return it.s * (n_iter + 1); }
  __device__ int64_t out_step() const { return 1; }
};

// CAP: the band table's size, kMaxBands1D for the audio entries, kMaxBands3D for volumes
template <bool IDENT, int CAP>
__global__ void __launch_bounds__(256) k_rank_mask(int64_t sets, MaskBands<CAP> rb, const float* __restrict__ coeffs,
                                                   const int32_t* __restrict__ rank, int64_t rank_len,
                                                   const int32_t* __restrict__ pos, int64_t n_iter, int64_t n_comp,
                                                   int deletion, float* __restrict__ out) {
  const RankPolicy<IDENT> p{rank, rank_len, pos, n_iter, n_comp, deletion != 0};
  mask_expand(p, rb, sets, n_iter + 1, coeffs, out, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
              (int64_t)gridDim.x * blockDim.x);
}

template <int CAP>
int launch_rank_mask(bool ident, int64_t sets, int nbands, const int64_t* band_off, bool ptrs_aligned,
                     const float* coeffs, const int32_t* rank, int64_t rank_len, const int32_t* pos, int64_t n_iter,
                     int64_t n_comp, int deletion, float* out, hipStream_t st, const char* name) {
  MaskBands<CAP> rb{};
  const int64_t units = fill_mask_bands(rb, nbands, band_off, sets, ptrs_aligned);
  if (units == 0) return WAM_OK;
  const int64_t K = rb.off[rb.nbands];
  const int64_t M = n_iter + 1;
  if ((M + kMaskChunk - 1) / kMaskChunk > 65535) return WAM_ERR_INVALID_ARG;
  WamTimer tm(st, name, 4.0 * (sets * K + sets * rank_len + (ident ? 0 : K) + (double)sets * M * K));
  const dim3 grid(wam_grid(units, 256), (unsigned)((M + kMaskChunk - 1) / kMaskChunk));
  if (ident)
    hipLaunchKernelGGL((k_rank_mask<true, CAP>), grid, dim3(256), 0, st, sets, rb, coeffs, rank, rank_len, pos, n_iter,
                       n_comp, deletion, out);
  else
    hipLaunchKernelGGL((k_rank_mask<false, CAP>), grid, dim3(256), 0, st, sets, rb, coeffs, rank, rank_len, pos, n_iter,
                       n_comp, deletion, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

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

// ---- wam_waverec1_ranked's helpers. The rank of every coefficient's mask slot in coefficient order, once
// per set (k_rank_table of dwt2_plane.hip, for the sets of a 1D plan): what the fused synthesis reads at
// the coefficient's own offset.
__global__ void __launch_bounds__(256) k_rank_table1(int64_t sets, int64_t K, const int32_t* __restrict__ rank,
                                                     int64_t rank_len, const int32_t* __restrict__ pos,
                                                     int32_t* __restrict__ rtab) {
  const int64_t total = sets * K;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = t / K;
    rtab[t] = slot_rank(rank + s * rank_len, pos[t - s * K], rank_len);
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

// Which route a 1D plan takes by itself: the fused kernel wherever it applies. Its slowest round beat route
// 0's fastest (and the default layout's composition) at every filter length it serves, 2 to 20 taps, at c3's
// evaluation geometry with 1 and 8 clips (profiles/eval1d_ranked_kbench.txt).
constexpr bool kFused1IsDefault = true;

bool fused1_supported(const wam_plan* p) { return dwt1_syn_ranked_supported(p); }

// floats of route 0's masked coefficient sets, rounded up to 16 bytes: wam_waverec's own workspace follows
int64_t masked_elems1(const wam_plan* p, int64_t sets, int64_t n_iter) {
  return (sets * (n_iter + 1) * p->band_off[p->nbands] + 3) & ~(int64_t)3;
}
int64_t rank_table1_bytes(const wam_plan* p, int64_t sets) {
  return (sets * p->band_off[p->nbands] * (int64_t)sizeof(int32_t) + 15) & ~(int64_t)15;
}

}  // namespace

// wam_rank_mask_coeffs's expansion over the bands of a 3D plan (evaluate3d.hip, route 0)
int launch_rank_mask_coeffs3(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* rank,
                             int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion,
                             float* out, hipStream_t st) {
  if (p->ndim != 3 || p->nbands > kMaxBands3D) return WAM_ERR_UNSUPPORTED;
  const bool ptrs_aligned = aligned16(coeffs) && aligned16(pos) && aligned16(out);
  return launch_rank_mask<kMaxBands3D>(false, sets, p->nbands, p->band_off, ptrs_aligned, coeffs, rank, rank_len, pos,
                                       n_iter, n_comp, deletion, out, st, "k_rank_mask_coeffs3");
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
  return launch_rank_mask<kMaxBands1D>(false, sets, plan->nbands, plan->band_off, ptrs_aligned, coeffs, rank, rank_len,
                                       pos, n_iter, n_comp, deletion, out, (hipStream_t)stream, "k_rank_mask_coeffs");
}

int wam_rank_mask_rows(int64_t sets, int64_t len, const float* src, const int32_t* rank, int64_t n_iter,
                       int64_t n_comp, int deletion, float* out, void* stream) {
  if (sets < 0 || len < 1 || len > INT32_MAX || n_iter < 1 || n_comp < 0 || !src || !rank || !out)
    return WAM_ERR_INVALID_ARG;
  const int64_t band_off[2] = {0, len};
  return launch_rank_mask<kMaxBands1D>(true, sets, 1, band_off, aligned16(src) && aligned16(rank) && aligned16(out), src,
                                       rank, len, nullptr, n_iter, n_comp, deletion, out, (hipStream_t)stream,
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

int wam_waverec1_ranked_route(const wam_plan* p) {
  if (!p) return -WAM_ERR_INVALID_ARG;
  if (p->ndim != 1) return -WAM_ERR_UNSUPPORTED;
  return kFused1IsDefault && fused1_supported(p) ? 1 : 0;
}

size_t wam_waverec1_ranked_workspace_bytes(const wam_plan* p, int64_t sets, int64_t n_iter, int route) {
  if (!p || p->ndim != 1 || sets < 0 || n_iter < 1 || route < -1 || route > 1) return 0;
  if (route == 1) return (size_t)rank_table1_bytes(p, sets);
  // route 0, and the plan's own route: its fallback is route 0, whose workspace also holds route 1's table
  return (size_t)(masked_elems1(p, sets, n_iter) * (int64_t)sizeof(float) +
                  wam_plan_workspace_bytes(p, sets * (n_iter + 1)));
}

int wam_waverec1_ranked(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* rank, int64_t rank_len,
                        const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion, int route, float* out,
                        float* row_max, void* workspace, void* stream) {
  if (!p || sets < 0 || rank_len < 1 || n_iter < 1 || n_comp < 0 || !coeffs || !rank || !pos || !out)
    return WAM_ERR_INVALID_ARG;
  if (p->ndim != 1 || p->nbands > kMaxBands1D) return WAM_ERR_UNSUPPORTED;
  if (!p->d_filt || rank_len > INT32_MAX || route < -1 || route > 1) return WAM_ERR_INVALID_ARG;
  if (route == 1 && !fused1_supported(p)) return WAM_ERR_UNSUPPORTED;
  const int64_t M = n_iter + 1, K = p->band_off[p->nbands], rec_len = p->rec_shape[0];
  if ((M + kMaskChunk - 1) / kMaskChunk > 65535 || sets * M > INT32_MAX) return WAM_ERR_INVALID_ARG;
  if (sets == 0) return WAM_OK;
  if (!workspace || !aligned16(workspace)) return WAM_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool own = route < 0;
  if (own) route = wam_waverec1_ranked_route(p);
  if (route == 1) {
    int32_t* rtab = (int32_t*)workspace;
    {
      WamTimer tm(st, "k_rank_table1", 4.0 * (sets * (double)rank_len + K + 2.0 * sets * K));
      hipLaunchKernelGGL(k_rank_table1, dim3(wam_grid(sets * K, 256)), dim3(256), 0, st, sets, K, rank, rank_len, pos,
                         rtab);
      WAM_LAUNCH_CHECK();
    }
    if (row_max) WAM_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)row_max, (int)0xff800000 /* -inf */, sets * M, st));
    const int rc = launch_dwt1_tile_synthesis_ranked(p, sets, coeffs, rtab, rank_len, n_iter, n_comp, deletion, out,
                                                     row_max, st);
    // a call the fused launcher declines (more than INT32_MAX units) is the caller's error when the
    // route was forced; the plan's own route then runs route 0, whose workspace the caller sized
    if (rc != WAM_ERR_UNSUPPORTED || !own) return rc;
  }
  float* masked = (float*)workspace;
  const bool ptrs_aligned = aligned16(coeffs) && aligned16(pos);
  if (int rc = launch_rank_mask<kMaxBands1D>(false, sets, p->nbands, p->band_off, ptrs_aligned, coeffs, rank, rank_len,
                                             pos, n_iter, n_comp, deletion, masked, st, "k_rank_mask_coeffs"))
    return rc;
  if (int rc = wam_waverec(p, sets * M, masked, nullptr, 1, out, masked + masked_elems1(p, sets, n_iter), stream))
    return rc;
  if (row_max) {
    const int vec = (rec_len & 3) == 0 && aligned16(out);
    WamTimer tm(st, "k_row_max", 4.0 * sets * M * rec_len);
    hipLaunchKernelGGL(k_row_max, dim3((unsigned)(sets * M)), dim3(rec_len >= 16384 ? 1024 : 256), 0, st, rec_len, out,
                       row_max, vec);
    WAM_LAUNCH_CHECK();
  }
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
