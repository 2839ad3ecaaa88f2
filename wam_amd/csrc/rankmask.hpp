// The ranking-driven mask expansion (mask_expand with a rank policy) behind wam_rank_mask_coeffs,
// wam_rank_mask_rows (evaluate1d.hip) and route 0 of the three ranked syntheses (evaluate_ranked.hip).
#pragma once
#include "maskexpand.hpp"

// mask_expand's policy: an element's fate is the rank of its mask slot pos[k] in its item's rank row.
// IDENT: the slot of element k is k (wam_rank_mask_rows), pos is not read.
// PLANES: item i is plane (image n = i / channels, channel c) and shares image n's rank row; its masked
// copies are planes (n, m, c) = (n * M + m) * channels + c of the output (2D). Otherwise item s is set s
// with its own row, its copies are s * M + m, and `channels` is not read: no division is compiled.
template <bool IDENT, bool PLANES>
struct RankPolicy {
  const int32_t* __restrict__ rank;
  int64_t rank_len;
  const int32_t* __restrict__ pos;
  int64_t n_iter, n_comp;
  int channels;
  bool del;
  struct Item { int64_t out0; const int32_t* rk; };  // the output item of mask 0 and the rank row
  using Elem = int32_t;
  using Mask = int64_t;
  __device__ Item item(int64_t i) const {
    if constexpr (PLANES) {
      const int64_t n = i / channels;
      return {n * (n_iter + 1) * channels + (i - n * channels), rank + n * rank_len};
    } else {
      return {i * (n_iter + 1), rank + i * rank_len};
    }
  }
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
  __device__ int64_t out_item(const Item& it) const { return it.out0; }
  __device__ int64_t out_step() const { return PLANES ? channels : 1; }
};

// CAP: the band table's size. `channels` is read with PLANES only.
template <bool IDENT, bool PLANES, int CAP>
__global__ void __launch_bounds__(256) k_rank_mask(int64_t items, MaskBands<CAP> rb, const float* __restrict__ coeffs,
                                                   const int32_t* __restrict__ rank, int64_t rank_len,
                                                   const int32_t* __restrict__ pos, int64_t n_iter, int64_t n_comp,
                                                   int deletion, int channels, float* __restrict__ out) {
  const RankPolicy<IDENT, PLANES> p{rank, rank_len, pos, n_iter, n_comp, channels, deletion != 0};
  mask_expand(p, rb, items, n_iter + 1, coeffs, out, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
              (int64_t)gridDim.x * blockDim.x);
}

// items = sets, or images * channels planes with PLANES; rank holds items / channels rows. `name`: the
// WamTimer label. More than 65535 chunks of kMaskChunk masks: WAM_ERR_INVALID_ARG, nothing launched.
template <int CAP, bool PLANES = false>
int launch_rank_mask(bool ident, int64_t items, int channels, int nbands, const int64_t* band_off, bool ptrs_aligned,
                     const float* coeffs, const int32_t* rank, int64_t rank_len, const int32_t* pos, int64_t n_iter,
                     int64_t n_comp, int deletion, float* out, hipStream_t st, const char* name) {
  MaskBands<CAP> rb{};
  const int64_t units = fill_mask_bands(rb, nbands, band_off, items, ptrs_aligned);
  if (units == 0) return WAM_OK;
  const int64_t K = rb.off[rb.nbands];
  const int64_t M = n_iter + 1, rows = items / channels;
  if ((M + kMaskChunk - 1) / kMaskChunk > 65535) return WAM_ERR_INVALID_ARG;
  WamTimer tm(st, name, 4.0 * (items * K + rows * rank_len + (ident ? 0 : K) + (double)items * M * K));
  const dim3 grid(wam_grid(units, 256), (unsigned)((M + kMaskChunk - 1) / kMaskChunk));
  if (ident && !PLANES)
    hipLaunchKernelGGL((k_rank_mask<true, false, CAP>), grid, dim3(256), 0, st, items, rb, coeffs, rank, rank_len, pos,
                       n_iter, n_comp, deletion, 1, out);
  else
    hipLaunchKernelGGL((k_rank_mask<false, PLANES, CAP>), grid, dim3(256), 0, st, items, rb, coeffs, rank, rank_len,
                       pos, n_iter, n_comp, deletion, channels, out);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}
