// Ranked synthesis: the n_iter + 1 masked reconstructions of every item straight from a ranking, the
// step between wam_wavedec and the model in Eval1DWAM (mask_layout="coeffs"), Eval2DWAM
// (mask_layout="mosaic") and Eval3DWAM. One host core serves wam_waverec1_ranked, wam_waverec2_ranked and
// wam_waverec_ranked; what differs between the dimensions is the RankedDim table below. Two routes give
// the same bits:
//   route 0: the shared mask expansion (rankmask.hpp) writes the masked coefficient sets band-major into
//     the caller's workspace and the plan's own wam_waverec reads them: any plan, about three times the
//     output's bytes of traffic;
//   route 1: a fused kernel applies the rank threshold as the synthesis loads its coefficients
//     (k_dwt1_syn_ranked, k_plane_syn_ranked, k_haar3_syn_ranked): no masked coefficient is stored.
#include "rankmask.hpp"

namespace {

// One call's arguments. items: sets (1D, 3D) or images (2D), each with one rank row; channels planes per item.
struct RankedCall {
  const wam_plan* p;
  int64_t items;
  int channels;
  const float* coeffs;
  const int32_t* rank;
  int64_t rank_len;
  const int32_t* pos;
  int64_t n_iter, n_comp;
  int deletion;
  float* out;
  float* row_max;  // 1D only, may be NULL
  hipStream_t st;
};

// What a dimension's entries differ in.
struct RankedDim {
  int ndim;
  int band_cap;  // the expansion's band table; a plan with more bands is WAM_ERR_UNSUPPORTED
  // Route 1 reads the ranks in coefficient order (k_rank_table) from items * K int32 of workspace. Then
  // every route needs a workspace: a NULL or misaligned one is WAM_ERR_INVALID_ARG before any launch, and
  // workspace_bytes(route -1) is route 0's size, the fallback's, which holds the table too. Without a
  // table route 1 reads no workspace: workspace_bytes(-1) is the own route's size (0 where fused), only
  // route 0 checks the workspace, and a fused decline on the own route with no workspace returns as it is.
  bool rank_table;
  // more than 65535 chunks of masks or INT32_MAX output rows: WAM_ERR_INVALID_ARG up front on every
  // route (1D: k_row_max's grid); otherwise each route's launcher states its own limit
  bool limits_up_front;
  bool (*fused_ok)(const wam_plan*);                       // the plans route 1 serves
  int (*fused)(const RankedCall&, const int32_t* rtab);    // WAM_ERR_UNSUPPORTED: declined, nothing launched
  int (*expand)(const RankedCall&, float* masked);         // route 0's first half
};

// Which route a plan takes by itself: the fused kernel wherever it applies. It measured faster in every
// dimension at the evaluators' geometries (profiles/eval1d_ranked_kbench.txt, eval2d_kbench.txt,
// eval3d_kbench.txt; DESIGN.md sections 3.13 to 3.15).
constexpr bool kFusedIsDefault = true;

bool aligned_in(const RankedCall& c) { return aligned16(c.coeffs) && aligned16(c.pos); }

template <int CAP, bool PLANES>
int expand(const RankedCall& c, float* masked, const char* name) {
  return launch_rank_mask<CAP, PLANES>(false, c.items * c.channels, c.channels, c.p->nbands, c.p->band_off,
                                       aligned_in(c), c.coeffs, c.rank, c.rank_len, c.pos, c.n_iter, c.n_comp,
                                       c.deletion, masked, c.st, name);
}

const RankedDim kDim1{
    1, 1 + WAM_MAX_LEVELS, /* rank_table */ true, /* limits_up_front */ true, dwt1_syn_ranked_supported,
    [](const RankedCall& c, const int32_t* rtab) {
      return launch_dwt1_tile_synthesis_ranked(c.p, c.items, c.coeffs, rtab, c.rank_len, c.n_iter, c.n_comp, c.deletion,
                                               c.out, c.row_max, c.st);
    },
    [](const RankedCall& c, float* masked) {
      return expand<1 + WAM_MAX_LEVELS, false>(c, masked, "k_rank_mask_coeffs");
    }};

const RankedDim kDim2{
    2, WAM_MAX_BANDS, /* rank_table */ true, /* limits_up_front */ false,
    [](const wam_plan* p) { return p->ndim == 2 && p->routes.syn == WAM_WHOLE_PLANE; },
    [](const RankedCall& c, const int32_t* rtab) {
      return launch_dwt2_plane_synthesis_ranked(c.p, c.items, c.channels, c.coeffs, rtab, c.rank_len, c.n_iter,
                                                c.n_comp, c.deletion, c.out, c.st);
    },
    [](const RankedCall& c, float* masked) { return expand<WAM_MAX_BANDS, true>(c, masked, "k_rank_mask2"); }};

const RankedDim kDim3{
    3, WAM_MAX_BANDS, /* rank_table */ false, /* limits_up_front */ false,
    [](const wam_plan* p) { return p->ndim == 3 && p->routes.syn == WAM_WHOLE_HAAR3; },
    [](const RankedCall& c, const int32_t*) {
      return launch_dwt3_haar_synthesis_ranked(c.p, c.items, c.coeffs, c.rank, c.rank_len, c.pos, c.n_iter, c.n_comp,
                                               c.deletion, c.out, c.st);
    },
    [](const RankedCall& c, float* masked) { return expand<WAM_MAX_BANDS, false>(c, masked, "k_rank_mask_coeffs3"); }};

// The rank of every coefficient's mask slot in coefficient order, once per item: what the fused 1D and 2D
// syntheses read at the coefficient's own offset.
__global__ void __launch_bounds__(256) k_rank_table(int64_t items, int64_t K, const int32_t* __restrict__ rank,
                                                    int64_t rank_len, const int32_t* __restrict__ pos,
                                                    int32_t* __restrict__ rtab) {
  const int64_t total = items * K;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = t / K;
    rtab[t] = slot_rank(rank + s * rank_len, pos[t - s * K], rank_len);
  }
}

int launch_rank_table(const RankedCall& c, int32_t* rtab) {
  const int64_t K = c.p->band_off[c.p->nbands];
  WamTimer tm(c.st, "k_rank_table", 4.0 * (c.items * (double)c.rank_len + K + 2.0 * c.items * K));
  hipLaunchKernelGGL(k_rank_table, dim3(wam_grid(c.items * K, 256)), dim3(256), 0, c.st, c.items, K, c.rank, c.rank_len,
                     c.pos, rtab);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int64_t rank_table_bytes(const wam_plan* p, int64_t items) {
  return (items * p->band_off[p->nbands] * (int64_t)sizeof(int32_t) + 15) & ~(int64_t)15;
}

// floats of route 0's masked coefficient sets, rounded up to 16 bytes: wam_waverec's own workspace follows
int64_t masked_elems(const wam_plan* p, int64_t out_items) {
  return (out_items * p->band_off[p->nbands] + 3) & ~(int64_t)3;
}

// ---- the core: route query, workspace size, call

int ranked_route(const RankedDim& d, const wam_plan* p) {
  if (!p) return -WAM_ERR_INVALID_ARG;
  if (p->ndim != d.ndim) return -WAM_ERR_UNSUPPORTED;
  return kFusedIsDefault && d.fused_ok(p) ? 1 : 0;
}

size_t ranked_workspace_bytes(const RankedDim& d, const wam_plan* p, int64_t items, int channels, int64_t n_iter,
                              int route) {
  if (!p || p->ndim != d.ndim || items < 0 || channels < 1 || channels > 4 || n_iter < 1 || route < -1 || route > 1)
    return 0;
  if (route < 0 && !d.rank_table) route = ranked_route(d, p);
  if (route == 1) return d.rank_table ? (size_t)rank_table_bytes(p, items) : 0;
  // route 0, and the own route of a dimension with a rank table: route 0 is its fallback
  const int64_t out_items = items * channels * (n_iter + 1);
  return (size_t)(masked_elems(p, out_items) * (int64_t)sizeof(float) + wam_plan_workspace_bytes(p, out_items));
}

int ranked_call(const RankedDim& d, const RankedCall& c, int route, void* workspace) {
  const wam_plan* p = c.p;
  if (!p || c.items < 0 || c.channels < 1 || c.channels > 4 || c.rank_len < 1 || c.n_iter < 1 || c.n_comp < 0 ||
      !c.coeffs || !c.rank || !c.pos || !c.out)
    return WAM_ERR_INVALID_ARG;
  if (p->ndim != d.ndim || p->nbands > d.band_cap) return WAM_ERR_UNSUPPORTED;
  if (!p->d_filt || c.rank_len > INT32_MAX || route < -1 || route > 1) return WAM_ERR_INVALID_ARG;
  if (route == 1 && !d.fused_ok(p)) return WAM_ERR_UNSUPPORTED;
  const int64_t M = c.n_iter + 1, out_items = c.items * c.channels * M;
  if (d.limits_up_front && ((M + kMaskChunk - 1) / kMaskChunk > 65535 || out_items > INT32_MAX))
    return WAM_ERR_INVALID_ARG;
  if (c.items == 0) return WAM_OK;
  const bool ws_ok = workspace && aligned16(workspace);
  if (d.rank_table && !ws_ok) return WAM_ERR_INVALID_ARG;
  const bool own = route < 0;
  if (own) route = ranked_route(d, p);
  if (route == 1) {
    if (d.rank_table)
      if (int rc = launch_rank_table(c, (int32_t*)workspace)) return rc;
    if (c.row_max)
      WAM_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)c.row_max, (int)0xff800000 /* -inf */, out_items, c.st));
    const int rc = d.fused(c, (const int32_t*)workspace);
    // A call the fused launcher declines (pointers its vector accesses cannot take, more units than its
    // grid holds) is the caller's error when the route was forced. The plan's own route then runs route 0
    // in the workspace the caller sized for it; a dimension whose route 1 reads no workspace may have
    // been given none, and then the decline stands.
    if (rc != WAM_ERR_UNSUPPORTED || !own || !workspace) return rc;
  }
  if (!ws_ok) return WAM_ERR_INVALID_ARG;
  float* masked = (float*)workspace;
  if (int rc = d.expand(c, masked)) return rc;
  if (int rc = wam_waverec(p, out_items, masked, nullptr, 1, c.out, masked + masked_elems(p, out_items), c.st))
    return rc;
  return c.row_max ? launch_row_max(out_items, p->rec_shape[0], c.out, c.row_max, c.st) : WAM_OK;
}

}  // namespace

extern "C" {

int wam_waverec1_ranked_route(const wam_plan* p) { return ranked_route(kDim1, p); }
int wam_waverec2_ranked_route(const wam_plan* p) { return ranked_route(kDim2, p); }
int wam_waverec_ranked_route(const wam_plan* p) { return ranked_route(kDim3, p); }

size_t wam_waverec1_ranked_workspace_bytes(const wam_plan* p, int64_t sets, int64_t n_iter, int route) {
  return ranked_workspace_bytes(kDim1, p, sets, 1, n_iter, route);
}
size_t wam_waverec2_ranked_workspace_bytes(const wam_plan* p, int64_t images, int channels, int64_t n_iter,
                                           int route) {
  return ranked_workspace_bytes(kDim2, p, images, channels, n_iter, route);
}
size_t wam_waverec_ranked_workspace_bytes(const wam_plan* p, int64_t sets, int64_t n_iter, int route) {
  return ranked_workspace_bytes(kDim3, p, sets, 1, n_iter, route);
}

int wam_waverec1_ranked(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* rank, int64_t rank_len,
                        const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion, int route, float* out,
                        float* row_max, void* workspace, void* stream) {
  return ranked_call(kDim1, {p, sets, 1, coeffs, rank, rank_len, pos, n_iter, n_comp, deletion, out, row_max,
                             (hipStream_t)stream}, route, workspace);
}
int wam_waverec2_ranked(const wam_plan* p, int64_t images, int channels, const float* coeffs, const int32_t* rank,
                        int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion, int route,
                        float* out, void* workspace, void* stream) {
  return ranked_call(kDim2, {p, images, channels, coeffs, rank, rank_len, pos, n_iter, n_comp, deletion, out, nullptr,
                             (hipStream_t)stream}, route, workspace);
}
int wam_waverec_ranked(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* rank, int64_t rank_len,
                       const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion, int route, float* out,
                       void* workspace, void* stream) {
  return ranked_call(kDim3, {p, sets, 1, coeffs, rank, rank_len, pos, n_iter, n_comp, deletion, out, nullptr,
                             (hipStream_t)stream}, route, workspace);
}

}  // extern "C"
