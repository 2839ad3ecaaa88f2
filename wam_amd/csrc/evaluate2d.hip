// Insertion / deletion of image WAMs by ranking (Eval2DWAM, mask_layout="mosaic"): the
// ranking-to-reconstruction step between wam_wavedec and the quantisation. Per image the n_iter + 1
// masked coefficient sets of its channel planes are reconstructed, [images, n_iter + 1, channels, H, W].
// Route 0 builds them with the shared mask expansion (maskexpand.hpp, k_rank_mask2 over the 1 + 3 J
// bands of the plan) in the caller's workspace and runs the plan's own synthesis: any 2D plan, about
// 3 M C H W floats of traffic per image (M = n_iter + 1). Route 1 (k_plane_syn_ranked, dwt2_plane.hip)
// applies the rank threshold as the plane-resident synthesis loads its coefficient rows: the M C H W
// output floats plus coefficients and ranks from L2. The two routes give the same bits.
#include "maskexpand.hpp"

namespace {

// Which route a plan takes by itself: the fused kernel wherever it applies. Its slowest round beat the
// fastest round of the composition it replaces (wam_rank_masks, wam_coeff_masks, wam_waverec) at haar and
// db4 J = 3 on 224 x 224, 1 and 4 images (profiles/eval2d_kbench.txt).
constexpr bool kFusedIsDefault = true;

bool fused_supported(const wam_plan* p) { return p->ndim == 2 && p->routes.syn == WAM_WHOLE_PLANE; }

// mask_expand's policy: plane i = (image n, channel c) shares image n's rank row; its masked copies
// are planes (n, m, c) = (n * M + m) * C + c of the output.
struct Rank2Policy {
  const int32_t* __restrict__ rank;
  int64_t rank_len;
  const int32_t* __restrict__ pos;
  int64_t n_iter, n_comp;
  int channels;
  bool del;
  struct Item { int64_t out0; const int32_t* rk; };
  using Elem = int32_t;
  using Mask = int64_t;
  __device__ Item item(int64_t i) const {
    const int64_t n = i / channels;
    return {n * (n_iter + 1) * channels + (i - n * channels), rank + n * rank_len};
  }
  template <int W>
  __device__ void load(const Item& it, int64_t bo, int64_t e, Elem (&rk)[W]) const {
    int32_t p[W];
    load_w<W>(pos + bo + e, p);
#pragma unroll
    for (int k = 0; k < W; ++k) rk[k] = slot_rank(it.rk, p[k], rank_len);
  }
  __device__ Mask mask(const Item&, int64_t m) const { return mask_thr(m, n_iter, n_comp, rank_len); }
  __device__ float keep(Mask thr, Elem rk) const { return (((int64_t)rk < thr) != del) ? 1.f : 0.f; }
  __device__ int64_t out_item(const Item& it) const { return it.out0; }
  __device__ int64_t out_step() const { return channels; }
};

__global__ void __launch_bounds__(256) k_rank_mask2(int64_t planes, MaskBands<WAM_MAX_BANDS> rb,
                                                    const float* __restrict__ coeffs, Rank2Policy p,
                                                    float* __restrict__ out) {
  mask_expand(p, rb, planes, p.n_iter + 1, coeffs, out, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
              (int64_t)gridDim.x * blockDim.x);
}

// floats of route 0's masked coefficient sets, rounded up to 16 bytes: wam_waverec's own workspace follows
int64_t masked_elems(const wam_plan* p, int64_t planes, int64_t n_iter) {
  return (planes * (n_iter + 1) * p->band_off[p->nbands] + 3) & ~(int64_t)3;
}

}  // namespace

extern "C" {

int wam_waverec2_ranked_route(const wam_plan* p) {
  if (!p) return -WAM_ERR_INVALID_ARG;
  if (p->ndim != 2) return -WAM_ERR_UNSUPPORTED;
  return kFusedIsDefault && fused_supported(p) ? 1 : 0;
}

size_t wam_waverec2_ranked_workspace_bytes(const wam_plan* p, int64_t images, int channels, int64_t n_iter,
                                           int route) {
  if (!p || p->ndim != 2 || images < 0 || channels < 1 || channels > 4 || n_iter < 1 || route < -1 || route > 1)
    return 0;
  if (route == 1) return (size_t)dwt2_plane_ranked_table_bytes(p, images);
  // route 0, and the plan's own route: its fallback is route 0, whose workspace also holds route 1's table
  const int64_t planes = images * channels;
  return (size_t)(masked_elems(p, planes, n_iter) * (int64_t)sizeof(float) +
                  wam_plan_workspace_bytes(p, planes * (n_iter + 1)));
}

int wam_waverec2_ranked(const wam_plan* p, int64_t images, int channels, const float* coeffs, const int32_t* rank,
                        int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion, int route,
                        float* out, void* workspace, void* stream) {
  if (!p || images < 0 || channels < 1 || channels > 4 || rank_len < 1 || n_iter < 1 || n_comp < 0 || !coeffs ||
      !rank || !pos || !out)
    return WAM_ERR_INVALID_ARG;
  if (p->ndim != 2) return WAM_ERR_UNSUPPORTED;
  if (!p->d_filt || rank_len > INT32_MAX || route < -1 || route > 1) return WAM_ERR_INVALID_ARG;
  if (route == 1 && !fused_supported(p)) return WAM_ERR_UNSUPPORTED;
  if (p->nbands > WAM_MAX_BANDS) return WAM_ERR_UNSUPPORTED;
  if (images == 0) return WAM_OK;
  if (!workspace || !aligned16(workspace)) return WAM_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool own = route < 0;
  if (own) route = wam_waverec2_ranked_route(p);
  if (route == 1) {
    const int rc = launch_dwt2_plane_synthesis_ranked(p, images, channels, coeffs, rank, rank_len, pos, n_iter, n_comp,
                                                      deletion, out, (int32_t*)workspace, st);
    // a call the fused launcher declines (an `out` its float2 stores cannot take) is the caller's
    // error when the route was forced; the plan's own route then runs route 0
    if (rc != WAM_ERR_UNSUPPORTED || !own) return rc;
  }
  const int64_t planes = images * channels, M = n_iter + 1;
  if ((M + kMaskChunk - 1) / kMaskChunk > 65535) return WAM_ERR_INVALID_ARG;
  float* masked = (float*)workspace;
  MaskBands<WAM_MAX_BANDS> rb{};
  const bool ptrs_aligned = aligned16(coeffs) && aligned16(pos);
  const int64_t units = fill_mask_bands(rb, p->nbands, p->band_off, planes, ptrs_aligned);
  const int64_t K = p->band_off[p->nbands];
  if (units) {
    WamTimer tm(st, "k_rank_mask2", 4.0 * (planes * K + images * rank_len + K + (double)planes * M * K));
    const Rank2Policy pol{rank, rank_len, pos, n_iter, n_comp, channels, deletion != 0};
    hipLaunchKernelGGL(k_rank_mask2, dim3(wam_grid(units, 256), (unsigned)((M + kMaskChunk - 1) / kMaskChunk)),
                       dim3(256), 0, st, planes, rb, coeffs, pol, masked);
    WAM_LAUNCH_CHECK();
  }
  return wam_waverec(p, planes * M, masked, nullptr, 1, out, masked + masked_elems(p, planes, n_iter), stream);
}

}  // extern "C"
