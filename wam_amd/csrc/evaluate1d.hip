// Audio insertion / deletion / faithfulness of spectra / input fidelity (Eval1DWAM,
// src/evaluators.py:39-306): the ranking-to-masked-input path between wam_wavedec and wam_waverec,
// and the peak normalisation between wam_waverec and the mel front-end. Per clip the reference
// builds n_iter + 1 masks on the host, multiplies them into the coefficients band by band, runs a
// float64 pywt.waverec of every masked set and divides each reconstruction by its maximum in numpy.
// Here the masks are never stored: one pass turns the ranking into the masked band-major
// coefficients of every (clip, mask) item wam_waverec reads, and one workgroup per reconstruction
// does the max reduction and the division. All three kernels are HBM-bound streaming passes.
#include "kernels.hpp"

namespace {

constexpr int kMaskChunk = 16;               // masks per blockIdx.y (the coefficient is re-read from L2)
constexpr int kMaxBands1D = 1 + WAM_MAX_LEVELS;

struct RankBands {
  int nbands;
  int vec[kMaxBands1D];         // band offset and length are multiples of 4 floats: 16-byte path
  int64_t off[kMaxBands1D + 1];   // per-item element offsets
  int64_t unit0[kMaxBands1D + 1]; // first work unit of the band (a unit = 4 elements, or 1 on the scalar path)
};

__device__ __forceinline__ int64_t mask_thr(int64_t m, int64_t n_iter, int64_t n_comp, int64_t rank_len) {
  if (m == 0) return 0;
  if (m >= n_iter) return rank_len;
  const int64_t t = m * n_comp;
  return t < rank_len ? t : rank_len;
}

// a mask slot outside [0, rank_len) is the pad column: rank -1, below every threshold
__device__ __forceinline__ int32_t slot_rank(const int32_t* __restrict__ rank, int32_t p, int64_t rank_len) {
  return ((uint64_t)(int64_t)p < (uint64_t)rank_len) ? rank[p] : -1;
}

// One thread owns 4 consecutive coefficients of one (band, set) (1 on the scalar path): it reads
// them, their mask slots and the slots' ranks once, and writes them into the kMaskChunk mask items of
// its blockIdx.y. For one mask a wave writes 64 x 16 consecutive bytes. IDENT: the slot of element k
// is k (wam_rank_mask_rows), pos is not read.
template <bool IDENT>
__global__ void __launch_bounds__(256) k_rank_mask(int64_t sets, RankBands rb, const float* __restrict__ coeffs,
                                                   const int32_t* __restrict__ rank, int64_t rank_len,
                                                   const int32_t* __restrict__ pos, int64_t n_iter, int64_t n_comp,
                                                   int deletion, float* __restrict__ out) {
  const int64_t M = n_iter + 1;
  const int64_t m0 = (int64_t)blockIdx.y * kMaskChunk;
  const int64_t m1 = m0 + kMaskChunk < M ? m0 + kMaskChunk : M;
  const bool del = deletion != 0;
  const int64_t units = rb.unit0[rb.nbands];
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    int b = 0;
#pragma unroll 1
    while (b + 1 < rb.nbands && u >= rb.unit0[b + 1]) ++b;
    const int64_t bo = rb.off[b], bn = rb.off[b + 1] - bo;
    const int64_t r = u - rb.unit0[b];
    if (rb.vec[b]) {
      const int64_t per = bn >> 2;
      const int64_t s = r / per, e = (r - s * per) << 2;
      const wam_f4v c = *reinterpret_cast<const wam_f4v*>(coeffs + sets * bo + s * bn + e);
      const int32_t* rk_s = rank + s * rank_len;
      int32_t rk[4];
      if (IDENT) {
        const int4 q = *reinterpret_cast<const int4*>(rk_s + e);
        rk[0] = q.x, rk[1] = q.y, rk[2] = q.z, rk[3] = q.w;
      } else {
        const int4 p = *reinterpret_cast<const int4*>(pos + bo + e);
        rk[0] = slot_rank(rk_s, p.x, rank_len);
        rk[1] = slot_rank(rk_s, p.y, rank_len);
        rk[2] = slot_rank(rk_s, p.z, rank_len);
        rk[3] = slot_rank(rk_s, p.w, rank_len);
      }
      float* o = out + sets * M * bo + s * M * bn + e;
      for (int64_t m = m0; m < m1; ++m) {
        const int64_t thr = mask_thr(m, n_iter, n_comp, rank_len);
        wam_f4v v;
        v.x = c.x * ((((int64_t)rk[0] < thr) != del) ? 1.f : 0.f);
        v.y = c.y * ((((int64_t)rk[1] < thr) != del) ? 1.f : 0.f);
        v.z = c.z * ((((int64_t)rk[2] < thr) != del) ? 1.f : 0.f);
        v.w = c.w * ((((int64_t)rk[3] < thr) != del) ? 1.f : 0.f);
        *reinterpret_cast<wam_f4v*>(o + m * bn) = v;
      }
    } else {
      const int64_t s = r / bn, e = r - s * bn;
      const float c = coeffs[sets * bo + s * bn + e];
      const int32_t rk = IDENT ? rank[s * rank_len + e] : slot_rank(rank + s * rank_len, pos[bo + e], rank_len);
      float* o = out + sets * M * bo + s * M * bn + e;
      for (int64_t m = m0; m < m1; ++m) {
        const int64_t thr = mask_thr(m, n_iter, n_comp, rank_len);
        o[m * bn] = c * ((((int64_t)rk < thr) != del) ? 1.f : 0.f);
      }
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_rank_mask(bool ident, int64_t sets, RankBands& rb, bool ptrs_aligned, const float* coeffs,
                     const int32_t* rank, int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp,
                     int deletion, float* out, hipStream_t st, const char* name) {
  int64_t units = 0;
  for (int b = 0; b < rb.nbands; ++b) {
    const int64_t bn = rb.off[b + 1] - rb.off[b];
    rb.vec[b] = ptrs_aligned && (rb.off[b] & 3) == 0 && (bn & 3) == 0;
    rb.unit0[b] = units;
    units += sets * (rb.vec[b] ? bn >> 2 : bn);
  }
  rb.unit0[rb.nbands] = units;
  if (units == 0) return WAM_OK;
  const int64_t K = rb.off[rb.nbands];
  const int64_t M = n_iter + 1;
  if ((M + kMaskChunk - 1) / kMaskChunk > 65535) return WAM_ERR_INVALID_ARG;
  WamTimer tm(st, name, 4.0 * (sets * K + sets * rank_len + (ident ? 0 : K) + (double)sets * M * K));
  const dim3 grid(wam_grid(units, 256), (unsigned)((M + kMaskChunk - 1) / kMaskChunk));
  if (ident)
    hipLaunchKernelGGL(k_rank_mask<true>, grid, dim3(256), 0, st, sets, rb, coeffs, rank, rank_len, pos, n_iter,
                       n_comp, deletion, out);
  else
    hipLaunchKernelGGL(k_rank_mask<false>, grid, dim3(256), 0, st, sets, rb, coeffs, rank, rank_len, pos, n_iter,
                       n_comp, deletion, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

// ---- out = in / max(in), one workgroup per row: wave-64 shuffles, one LDS step, 16-byte loads when
// the rows are 16-byte aligned; the second read of the row comes from L2.
__device__ __forceinline__ float block_max(float mx) {
  __shared__ float smx[16];
  for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) smx[w] = mx;
  __syncthreads();
  mx = smx[0];
  for (int i = 1; i < nw; ++i) mx = fmaxf(mx, smx[i]);
  return mx;
}

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
  mx = block_max(mx);
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

}  // namespace

extern "C" {

int wam_rank_mask_coeffs(const wam_plan* plan, int64_t sets, const float* coeffs, const int32_t* rank,
                         int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion,
                         float* out, void* stream) {
  if (!plan || sets < 0 || rank_len < 1 || n_iter < 1 || n_comp < 0 || !coeffs || !rank || !pos || !out)
    return WAM_ERR_INVALID_ARG;
  if (plan->ndim != 1 || plan->nbands > kMaxBands1D) return WAM_ERR_UNSUPPORTED;
  if (rank_len > INT32_MAX) return WAM_ERR_INVALID_ARG;
  RankBands rb{};
  rb.nbands = plan->nbands;
  for (int b = 0; b <= plan->nbands; ++b) rb.off[b] = plan->band_off[b];
  return launch_rank_mask(false, sets, rb, aligned16(coeffs) && aligned16(pos) && aligned16(out), coeffs, rank,
                          rank_len, pos, n_iter, n_comp, deletion, out, (hipStream_t)stream, "k_rank_mask_coeffs");
}

int wam_rank_mask_rows(int64_t sets, int64_t len, const float* src, const int32_t* rank, int64_t n_iter,
                       int64_t n_comp, int deletion, float* out, void* stream) {
  if (sets < 0 || len < 1 || len > INT32_MAX || n_iter < 1 || n_comp < 0 || !src || !rank || !out)
    return WAM_ERR_INVALID_ARG;
  RankBands rb{};
  rb.nbands = 1;
  rb.off[0] = 0;
  rb.off[1] = len;
  return launch_rank_mask(true, sets, rb, aligned16(src) && aligned16(rank) && aligned16(out), src, rank, len,
                          nullptr, n_iter, n_comp, deletion, out, (hipStream_t)stream, "k_rank_mask_rows");
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

}  // extern "C"
