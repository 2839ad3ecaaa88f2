// Insertion / deletion of voxel WAMs (Eval3DWAM): the ranking-to-reconstruction step between
// wam_wavedec and the model. Per source volume n_iter + 1 masked coefficient sets are reconstructed.
// Route 0 builds them with the shared mask expansion (maskexpand.hpp, k_rank_mask over the 1 + 7 J
// bands of the plan) in the caller's workspace and runs the plan's own synthesis: any 3D plan, about
// 3 M S^3 floats of traffic per volume (M = n_iter + 1). Route 1 (k_haar3_syn_ranked, dwt3_haar.hip)
// applies the rank threshold as the synthesis loads: no intermediate, the M S^3 output floats plus
// the coefficients, positions and ranks once per chunk of masks. The two routes give the same bits.
#include "kernels.hpp"

namespace {

// Which route a plan takes by itself: the fused kernel wherever it applies. It is the faster of the
// two at c5's geometry and at J = 1 (profiles/eval3d_kbench.txt).
constexpr bool kFusedIsDefault = true;

bool fused_supported(const wam_plan* p) { return p->ndim == 3 && p->routes.syn == WAM_WHOLE_HAAR3; }

// floats of route 0's masked coefficient sets, rounded up to 16 bytes: wam_waverec's own workspace follows
int64_t masked_elems(const wam_plan* p, int64_t sets, int64_t n_iter) {
  return (sets * (n_iter + 1) * p->band_off[p->nbands] + 3) & ~(int64_t)3;
}

}  // namespace

extern "C" {

int wam_waverec_ranked_route(const wam_plan* p) {
  if (!p) return -WAM_ERR_INVALID_ARG;
  if (p->ndim != 3) return -WAM_ERR_UNSUPPORTED;
  return kFusedIsDefault && fused_supported(p) ? 1 : 0;
}

size_t wam_waverec_ranked_workspace_bytes(const wam_plan* p, int64_t sets, int64_t n_iter, int route) {
  if (!p || p->ndim != 3 || sets < 0 || n_iter < 1 || route < -1 || route > 1) return 0;
  if (route < 0) route = wam_waverec_ranked_route(p);
  if (route == 1) return 0;
  return (size_t)(masked_elems(p, sets, n_iter) * (int64_t)sizeof(float) +
                  wam_plan_workspace_bytes(p, sets * (n_iter + 1)));
}

int wam_waverec_ranked(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* rank, int64_t rank_len,
                       const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion, int route, float* out,
                       void* workspace, void* stream) {
  if (!p || sets < 0 || rank_len < 1 || n_iter < 1 || n_comp < 0 || !coeffs || !rank || !pos || !out)
    return WAM_ERR_INVALID_ARG;
  if (p->ndim != 3) return WAM_ERR_UNSUPPORTED;
  if (!p->d_filt || rank_len > INT32_MAX || route < -1 || route > 1) return WAM_ERR_INVALID_ARG;
  if (route == 1 && !fused_supported(p)) return WAM_ERR_UNSUPPORTED;
  if (sets == 0) return WAM_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool own = route < 0;
  if (own) route = wam_waverec_ranked_route(p);
  if (route == 1) {
    const int rc = launch_dwt3_haar_synthesis_ranked(p, sets, coeffs, rank, rank_len, pos, n_iter, n_comp, deletion,
                                                     out, st);
    // a call the fused launcher declines (pointers its vector accesses cannot take) is the caller's
    // error when the route was forced; the plan's own route then runs route 0, given its workspace
    if (rc != WAM_ERR_UNSUPPORTED || !own || !workspace) return rc;
  }
  if (!workspace || ((uintptr_t)workspace & 15)) return WAM_ERR_INVALID_ARG;
  float* masked = (float*)workspace;
  const int rc = launch_rank_mask_coeffs3(p, sets, coeffs, rank, rank_len, pos, n_iter, n_comp, deletion, masked, st);
  if (rc) return rc;
  return wam_waverec(p, sets * (n_iter + 1), masked, nullptr, 1, out, masked + masked_elems(p, sets, n_iter), stream);
}

}  // extern "C"
