// The masked expansion shared by the evaluators' band-major mask kernels (rankmask.hpp: k_rank_mask,
// analyze2d.hip: k_threshold_mask): every coefficient of every input item is read once and written,
// times a 0 / 1 multiplier, into all the mask items wam_waverec reads -- the masks are never stored.
// mask_thr, kMaskChunk and aligned16 / aligned4 also serve baselines2d.hip and evaluate.hip.
#pragma once
#include "kernels.hpp"

constexpr int kMaskChunk = 16;  // masks per blockIdx.y: what a thread loaded for its elements stays in registers

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// generate_masks (src/evaluation_helpers.py:469-505): mask m keeps the ranks below thr(m): thr(0) = 0,
// thr(m) = m * n_comp (m < n_iter), thr(n_iter) = all `len` (the reference forces the last mask full)
__device__ __forceinline__ int64_t mask_thr(int64_t m, int64_t n_iter, int64_t n_comp, int64_t len) {
  if (m == 0) return 0;
  if (m >= n_iter) return len;
  const int64_t t = m * n_comp;
  return t < len ? t : len;
}

// the rank of mask slot p in a set's rank row; a slot outside [0, rank_len) is the pad column: rank -1,
// below every threshold
__device__ __forceinline__ int32_t slot_rank(const int32_t* __restrict__ rank, int32_t p, int64_t rank_len) {
  return ((uint64_t)(int64_t)p < (uint64_t)rank_len) ? rank[p] : -1;
}

template <int CAP>
struct MaskBands {
  int nbands;
  int vec[CAP];            // band offset and length are multiples of 4 floats: 16-byte path
  int64_t off[CAP + 1];    // per-item element offsets
  int64_t unit0[CAP + 1];  // first work unit of the band (a unit = 4 elements, or 1 on the scalar path)
};

// The table of `items` input items laid out by band_off[0 .. nbands]; returns the unit count.
template <int CAP>
int64_t fill_mask_bands(MaskBands<CAP>& mb, int nbands, const int64_t* band_off, int64_t items, bool ptrs_aligned) {
  mb.nbands = nbands;
  int64_t units = 0;
  for (int b = 0; b < nbands; ++b) {
    const int64_t bn = band_off[b + 1] - band_off[b];
    mb.off[b] = band_off[b];
    mb.vec[b] = ptrs_aligned && (band_off[b] & 3) == 0 && (bn & 3) == 0;
    mb.unit0[b] = units;
    units += items * (mb.vec[b] ? bn >> 2 : bn);
  }
  mb.off[nbands] = band_off[nbands];
  mb.unit0[nbands] = units;
  return units;
}

// W consecutive floats or int32 table entries: one 16-byte load on the vector path
template <int W, class T>
__device__ __forceinline__ void load_w(const T* __restrict__ src, T (&v)[W]) {
  if constexpr (W == 4) {
    typedef T v4 __attribute__((ext_vector_type(4)));
    const v4 q = *reinterpret_cast<const v4*>(src);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = src[0];
  }
}

// One unit: W consecutive coefficients of input item `item` of the band at bo, bn long. The policy P gives
//   Item item(i)                      what the item's elements share (its rank row, its map and threshold rows)
//   load<W>(item, bo, e, Elem[W])     what decides an element's fate, read once
//   Mask mask(item, m)                what mask m compares against, once per mask and not per element
//   float keep(Mask, Elem)            the 0 / 1 multiplier
//   int64_t out_item(item)            the output item of (item, mask 0) ...
//   int64_t out_step()                ... and how many output items lie between two masks of an item
// Input and output are band-major, items * bo + item * bn + e: for one mask a wave writes 64 x 16
// consecutive bytes on the vector path.
template <int W, class P>
__device__ __forceinline__ void mask_expand_unit(const P& p, int64_t items, int64_t out_items, int64_t bo, int64_t bn,
                                                 int64_t r, int64_t m0, int64_t m1, const float* __restrict__ coeffs,
                                                 float* __restrict__ out) {
  const int64_t per = W == 4 ? bn >> 2 : bn;
  const int64_t i = r / per, e = (r - i * per) * W;
  float c[W];
  load_w<W>(coeffs + items * bo + i * bn + e, c);
  const typename P::Item it = p.item(i);
  typename P::Elem el[W];
  p.template load<W>(it, bo, e, el);
  float* o = out + out_items * bo + p.out_item(it) * bn + e;
  const int64_t step = p.out_step() * bn;
  for (int64_t m = m0; m < m1; ++m) {
    const typename P::Mask mk = p.mask(it, m);
    float v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = c[k] * p.keep(mk, el[k]);
    float* dst = o + m * step;
    if constexpr (W == 4) *reinterpret_cast<wam_f4v*>(dst) = wam_f4v{v[0], v[1], v[2], v[3]};
    else dst[0] = v[0];
  }
}

// The kernel body: a grid-stride walk over the units of all bands, blockIdx.y picks the chunk of masks.
// The walk's `first` unit and `stride` (blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x)
// come from the __global__ function: only a blockDim read there is folded into a scalar load of the
// uniform workgroup size; read here it is a vector load and two more VGPRs.
template <class P, int CAP>
__device__ __forceinline__ void mask_expand(const P& p, const MaskBands<CAP>& mb, int64_t items, int64_t n_masks,
                                            const float* __restrict__ coeffs, float* __restrict__ out, int64_t first,
                                            int64_t stride) {
  const int64_t m0 = (int64_t)blockIdx.y * kMaskChunk;
  const int64_t m1 = m0 + kMaskChunk < n_masks ? m0 + kMaskChunk : n_masks;
  const int64_t units = mb.unit0[mb.nbands];
  for (int64_t u = first; u < units; u += stride) {
    int b = 0;
#pragma unroll 1
    while (b + 1 < mb.nbands && u >= mb.unit0[b + 1]) ++b;
    const int64_t bo = mb.off[b], bn = mb.off[b + 1] - bo;
    const int64_t r = u - mb.unit0[b];
    if (mb.vec[b]) mask_expand_unit<4>(p, items, items * n_masks, bo, bn, r, m0, m1, coeffs, out);
    else mask_expand_unit<1>(p, items, items * n_masks, bo, bn, r, m0, m1, coeffs, out);
  }
}
