// Cell-mask synthesis (wam_waverec_cells): the reconstructions of every volume under n_masks float-valued
// superpixel masks, the step between wam_wavedec and the model in Eval3DWAM.mu_fidelity. Every
// coefficient is multiplied by its grid cell's value of the mask (slot: coefficient -> cell, shared by all
// sets; a slot outside the grid multiplies by 1.0f). Two routes give the same bits, as the ranked
// syntheses' (evaluate_ranked.hip):
//   route 0: the shared mask expansion (maskexpand.hpp) with the cell policy below writes the masked sets
//     band-major into the caller's workspace and the plan's own wam_waverec reads them: any 3D plan;
//   route 1: k_haar3_syn_cells (dwt3_haar.hip) multiplies as the synthesis loads its coefficients: no
//     masked coefficient is stored.
#include "maskexpand.hpp"

namespace {

// Which route a plan takes by itself where route 1 serves it (profiles/eval3d_cells_kbench.txt, DESIGN.md
// section 3.19).
constexpr bool kFusedIsDefault = true;

// mask_expand's policy: an element's multiplier is its grid cell's value in the mask's row of the item's
// masks. Item s is set s with rows grid[s, 0 .. n_masks); its copies are output items s * n_masks + m.
struct CellPolicy {
  const int32_t* __restrict__ slot;
  const float* __restrict__ grid;
  int64_t n_masks, grid_len;
  struct Item { int64_t out0; const float* rows; };
  using Elem = int32_t;
  using Mask = const float*;
  __device__ Item item(int64_t i) const { return {i * n_masks, grid + i * n_masks * grid_len}; }
  template <int W>
  __device__ void load(const Item&, int64_t bo, int64_t e, Elem (&s)[W]) const { load_w<W>(slot + bo + e, s); }
  __device__ Mask mask(const Item& it, int64_t m) const { return it.rows + m * grid_len; }
  __device__ float keep(Mask row, Elem s) const { return ((uint64_t)(int64_t)s < (uint64_t)grid_len) ? row[s] : 1.f; }
  __device__ int64_t out_item(const Item& it) const { return it.out0; }
  __device__ int64_t out_step() const { return 1; }
};

__global__ void __launch_bounds__(256) k_cell_mask_coeffs3(int64_t items, MaskBands<WAM_MAX_BANDS> mb,
                                                           const float* __restrict__ coeffs,
                                                           const int32_t* __restrict__ slot, int64_t n_masks,
                                                           int64_t grid_len, const float* __restrict__ grid,
                                                           float* __restrict__ out) {
  const CellPolicy p{slot, grid, n_masks, grid_len};
  mask_expand(p, mb, items, n_masks, coeffs, out, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
              (int64_t)gridDim.x * blockDim.x);
}

int launch_cell_mask(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* slot, int64_t n_masks,
                     int64_t grid_len, const float* grid, float* masked, hipStream_t st) {
  MaskBands<WAM_MAX_BANDS> mb{};
  const int64_t units = fill_mask_bands(mb, p->nbands, p->band_off, sets, aligned16(coeffs) && aligned16(slot));
  if (units == 0) return WAM_OK;
  const double K = (double)mb.off[mb.nbands];
  WamTimer tm(st, "k_cell_mask_coeffs3", 4.0 * (sets * K + K + (double)sets * n_masks * (grid_len + K)));
  const dim3 gd(wam_grid(units, 256), (unsigned)((n_masks + kMaskChunk - 1) / kMaskChunk));
  hipLaunchKernelGGL(k_cell_mask_coeffs3, gd, dim3(256), 0, st, sets, mb, coeffs, slot, n_masks, grid_len, grid,
                     masked);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

bool fused_ok(const wam_plan* p) { return p->ndim == 3 && p->routes.syn == WAM_WHOLE_HAAR3; }

// floats of route 0's masked coefficient sets, rounded up to 16 bytes: wam_waverec's own workspace follows
int64_t masked_elems(const wam_plan* p, int64_t out_items) {
  return (out_items * p->band_off[p->nbands] + 3) & ~(int64_t)3;
}

}  // namespace

extern "C" {

int wam_waverec_cells_route(const wam_plan* p) {
  if (!p) return -WAM_ERR_INVALID_ARG;
  if (p->ndim != 3) return -WAM_ERR_UNSUPPORTED;
  return kFusedIsDefault && fused_ok(p) ? 1 : 0;
}

size_t wam_waverec_cells_workspace_bytes(const wam_plan* p, int64_t sets, int64_t n_masks, int route) {
  if (!p || p->ndim != 3 || sets < 0 || n_masks < 1 || route < -1 || route > 1) return 0;
  if (route < 0) route = wam_waverec_cells_route(p);
  if (route == 1) return 0;
  const int64_t out_items = sets * n_masks;
  return (size_t)(masked_elems(p, out_items) * (int64_t)sizeof(float) + wam_plan_workspace_bytes(p, out_items));
}

int wam_waverec_cells(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* slot, int64_t n_masks,
                      int64_t grid_len, const float* grid, int route, float* out, void* workspace, void* stream) {
  if (!p || sets < 0 || n_masks < 1 || grid_len < 1 || !coeffs || !slot || !grid || !out) return WAM_ERR_INVALID_ARG;
  if (p->ndim != 3 || p->nbands > WAM_MAX_BANDS) return WAM_ERR_UNSUPPORTED;
  if (!p->d_filt || route < -1 || route > 1) return WAM_ERR_INVALID_ARG;
  if (route == 1 && !fused_ok(p)) return WAM_ERR_UNSUPPORTED;
  if ((n_masks + kMaskChunk - 1) / kMaskChunk > 65535) return WAM_ERR_INVALID_ARG;
  if (sets == 0) return WAM_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool own = route < 0;
  if (own) route = wam_waverec_cells_route(p);
  if (route == 1) {
    const int rc = launch_dwt3_haar_synthesis_cells(p, sets, coeffs, slot, n_masks, grid_len, grid, out, st);
    // A call the fused launcher declines (a grid_len above its 16-bit columns, pointers its vector accesses
    // cannot take, more sets than its grid holds) is the caller's error when the route was forced. The plan's
    // own route then runs route 0 when a workspace was given; without one the decline stands.
    if (rc != WAM_ERR_UNSUPPORTED || !own || !workspace) return rc;
  }
  if (!workspace || !aligned16(workspace)) return WAM_ERR_INVALID_ARG;
  const int64_t out_items = sets * n_masks;
  float* masked = (float*)workspace;
  if (int rc = launch_cell_mask(p, sets, coeffs, slot, n_masks, grid_len, grid, masked, st)) return rc;
  return wam_waverec(p, out_items, masked, nullptr, 1, out, masked + masked_elems(p, out_items), st);
}

}  // extern "C"
