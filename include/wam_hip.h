/*
 * wam_hip.h -- C-ABI of libwam_hip.so, the MI355X (gfx950) kernels behind the WAM attribution path.
 *
 * The reference (michalpiasecki0/wam) is pure Python: its hot path calls the third-party ptwt
 * package (not vendored; ptwt>=0.1.0, de-facto 1.0.1) for every wavelet transform and numpy for
 * the per-subband post-processing. The entry points below replace exactly those calls; the
 * Python classes in wam_amd/ keep the reference's class / method signatures and bind these
 * symbols with ctypes (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - plain pointers + sizes only; every device buffer is allocated by the caller (torch);
 *   - every compute entry point is asynchronous on the given hipStream_t (passed as void*);
 *   - return value: 0 = success, otherwise a code for wam_strerror(); nothing throws;
 *   - plans are immutable after creation and may be shared by concurrent streams;
 *   - coefficient buffers are BAND-MAJOR: band b occupies [batch, band dims...] contiguously at
 *     element offset batch * wam_plan_band_offset(plan, b). Band order is ptwt's:
 *       1D: [A_J, D_J, ..., D_1]
 *       2D: [A_J, (H_J, V_J, D_J), ..., (H_1, V_1, D_1)]   H = hi along rows, lo along columns
 *       3D: [A_J, (aad, ada, add, daa, dad, dda, ddd)_J, ..., (...)_1]  letters = axes (-3,-2,-1)
 */
#ifndef WAM_HIP_H
#define WAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* boundary modes (ptwt names; 'constant' is ptwt's alias of torch 'replicate') */
enum wam_mode { WAM_MODE_ZERO = 0, WAM_MODE_REFLECT = 1, WAM_MODE_SYMMETRIC = 2,
                WAM_MODE_CONSTANT = 3, WAM_MODE_PERIODIC = 4 };

/* error codes (HIP runtime errors are returned as WAM_ERR_HIP_BASE + hipError_t) */
enum wam_status { WAM_OK = 0, WAM_ERR_INVALID_ARG = 1, WAM_ERR_SHAPE = 2, WAM_ERR_UNSUPPORTED = 3,
                  WAM_ERR_NO_MEMORY = 4, WAM_ERR_HIP_BASE = 1000 };

typedef struct wam_plan wam_plan;

const char* wam_strerror(int status);
/* library / ABI version; bumped on any signature change */
int wam_version(void);

/* ------------------------------------------------------------------------------------------------
 * Plans: one per (ndim, spatial shape, levels, filter bank, mode). Replaces ptwt's per-call
 * filter construction (_get_filter_tensors / _construct_{2,3}d_filt) and size bookkeeping
 * (_get_pad, _adjust_padding_at_reconstruction).
 * filters are pywt's float64 tables, cast to fp32 on the device (as ptwt casts to x.dtype).
 * ---------------------------------------------------------------------------------------------- */
int wam_plan_create(wam_plan** plan, int ndim, const int64_t* shape, int levels,
                    const double* dec_lo, const double* dec_hi,
                    const double* rec_lo, const double* rec_hi, int filt_len, int mode);
/* flags: WAM_PLAN_GENERIC forces the per-axis kernels, WAM_PLAN_NO_ROWS skips the row-resident
 * and plane-resident 2D kernels, WAM_PLAN_NO_PLANE skips only the plane-resident (all levels in
 * one workgroup) kernels; WAM_PLAN_NO_COOP / WAM_PLAN_FORCE_COOP pick the plane kernels' level-1
 * form (wave chunks / cooperative row stream) instead of the size-based choice (all used by tests to
 * cross-check the fused 2D kernels); 0 selects the fastest path. Bit 32 (a line-streaming analysis
 * that never beat the plane kernel) is retired and ignored.
 * wam_plan_create == wam_plan_create_ex(..., 0). */
enum wam_plan_flags { WAM_PLAN_GENERIC = 1, WAM_PLAN_NO_ROWS = 2, WAM_PLAN_NO_PLANE = 4, WAM_PLAN_NO_COOP = 8,
                      WAM_PLAN_FORCE_COOP = 16 };
int wam_plan_create_ex(wam_plan** plan, int ndim, const int64_t* shape, int levels,
                       const double* dec_lo, const double* dec_hi,
                       const double* rec_lo, const double* rec_hi, int filt_len, int mode, int flags);
/* a host-only plan: the same geometry, band layout, caps and workspace queries, no device (no
 * filters uploaded). Every compute entry point refuses it with WAM_ERR_INVALID_ARG. Used by the
 * sanitizer build of the host code (tests/native/). */
int wam_plan_create_host(wam_plan** plan, int ndim, const int64_t* shape, int levels,
                         const double* dec_lo, const double* dec_hi,
                         const double* rec_lo, const double* rec_hi, int filt_len, int mode, int flags);
void wam_plan_destroy(wam_plan* plan);
int wam_plan_num_bands(const wam_plan* plan);
/* dims of band b (ndim values) */
int wam_plan_band_shape(const wam_plan* plan, int band, int64_t* dims);
/* element offset of band b for ONE item (multiply by batch for a batched buffer) */
int64_t wam_plan_band_offset(const wam_plan* plan, int band);
/* coefficients per item (sum over bands) */
int64_t wam_plan_coeff_numel(const wam_plan* plan);
/* spatial dims produced by wam_waverec (ptwt: odd n reconstructs to n+1) */
int wam_plan_rec_shape(const wam_plan* plan, int64_t* dims);
/* bytes of scratch the transforms need for `batch` items (caller allocates). For 2D plans on the
 * per-level row synthesis it covers the intermediate approximations of 8 IG alphas, which
 * wam_waverec synthesises per level launch. */
int64_t wam_plan_workspace_bytes(const wam_plan* plan, int64_t batch);

/* ------------------------------------------------------------------------------------------------
 * Transforms
 * ---------------------------------------------------------------------------------------------- */
/* ptwt.wavedec / wavedec2 / wavedec3 (lib/wam_2D.py:96,430; lib/wam_1D.py:109,370;
 * lib/wam_3D.py:194,620). x: [batch, shape...]; coeffs: band-major, batch items. */
int wam_wavedec(const wam_plan* plan, int64_t batch, const float* x, float* coeffs,
                void* workspace, void* stream);

/* ptwt.waverec / waverec2 / waverec3 (lib/wam_2D.py:113; lib/wam_1D.py:117; lib/wam_3D.py:206,222)
 * with the Integrated-Gradients path scaling fused into the coefficient load
 * (lib/wam_2D.py:461-476 alter()): out[a, b] = waverec(fp32(alpha[a]) * coeffs[b]) for
 * a < n_alpha; alpha is a HOST array (alpha == NULL: n_alpha must be 1, no scaling).
 * out: [n_alpha, batch, rec_shape...]. */
int wam_waverec(const wam_plan* plan, int64_t batch, const float* coeffs, const float* alpha,
                int n_alpha, float* out, void* workspace, void* stream);

/* Adjoint of wam_waverec w.r.t. its coefficients = the backward pass of waverec in the
 * reference's loss.backward() (lib/wam_2D.py:116): zero-padded analysis with reverse(rec)
 * filters. grad: [batch, rec_shape...]; coeff_grads: band-major. */
int wam_waverec_adjoint(const wam_plan* plan, int64_t batch, const float* grad, float* coeff_grads,
                        void* workspace, void* stream);

/* Adjoint of wam_wavedec w.r.t. x (the backward pass of ptwt.wavedec*): coeff_grads band-major,
 * batch items -> grad_x [batch, shape...]. Per axis of a level it is the transposed convolution of
 * the band gradients with the analysis filters, its padded tails folded back onto the signal by the
 * plan's boundary mode (every mode, any length; an odd length does not grow). Outputs are gathered
 * in a fixed order, so two calls give the same bits. workspace: at least
 * wam_wavedec_adjoint_workspace_bytes (never more than wam_plan_workspace_bytes). */
int     wam_wavedec_adjoint(const wam_plan* plan, int64_t batch, const float* coeff_grads, float* grad_x,
                            void* workspace, void* stream);
int64_t wam_wavedec_adjoint_workspace_bytes(const wam_plan* plan, int64_t batch);
/* which kernels serve a level of wam_wavedec_adjoint: 0 = axis (per-axis kernels, every plan),
 * 1 = fold2d (2D, filter length <= 20, the level longer than the pad on both axes: streaming level
 * synthesis for the interior plus a border kernel for the folded tails); level 0 = finest; works on
 * host-only plans; negative on bad arguments */
int     wam_plan_wavedec_adjoint_route(const wam_plan* plan, int level);

/* ------------------------------------------------------------------------------------------------
 * Fused WAM passes (2D, rows <= 512 samples, filter length in {2,4,6,8,12,16,20})
 * ---------------------------------------------------------------------------------------------- */
enum wam_caps { WAM_CAP_NOISY_WAVEDEC = 1, WAM_CAP_ADJOINT_MAPS = 2, WAM_CAP_BF16_NHWC = 4 };
/* which fused entry points below this plan supports (bit set of wam_caps) */
int wam_plan_caps(const wam_plan* plan);
/* which kernel family serves each transform of this plan, as one NUL-terminated line in buf (cap
 * bytes; 512 hold any plan), e.g.
 *   ana=plane|rows,rows,rows adj=plane|rows,rows,rows syn=plane|colstrip maps=plane caps=7
 * ana (wam_wavedec), adj (wam_waverec_adjoint): the whole-transform route (none, plane, tile1,
 * haar3), then after '|' the route of every level, finest first (rows, colstrip, tile3, axis), which
 * serves plans without a whole-transform route and calls that route declines (e.g. a buffer that
 * is not 16-byte aligned); syn (wam_waverec): the same with one route for all levels; maps: the fused
 * wam_waverec_adjoint_maps pass (none, plane, rows); caps: wam_plan_caps. Works on host-only plans.
 * WAM_ERR_INVALID_ARG when buf is too small. */
int wam_plan_describe(const wam_plan* plan, char* buf, int cap);

/* SmoothGrad sample generation fused into the first analysis level (lib/wam_2D.py:390-406):
 * coeffs of x_i + sigma_i * N(0,1) for n_samples x images x channels planes, with the same
 * Philox stream as wam_noise_add (counter (sample_base + s, image, element / 4)), without
 * materialising the noisy input. x: [images, channels, H, W]; coeffs band-major over the
 * (sample, image, channel) planes. WAM_ERR_UNSUPPORTED unless WAM_CAP_NOISY_WAVEDEC. Also 3D Haar
 * plans (J <= 2, dims divisible by 2^J, W % 4 == 0; lib/wam_3D.py:565-582) for channels == 1:
 * x [images, 1, D, H, W], coeffs over the (sample, image) volumes. */
int wam_wavedec_noisy(const wam_plan* plan, int64_t n_samples, int64_t images, int channels,
                      const float* x, const float* sigma, uint64_t seed, int64_t sample_base,
                      float* coeffs, void* workspace, void* stream);
/* the same with the Philox image counter offset by image_base: x holds images [image_base,
 * image_base + images) of a batch sharded over ranks, so every image keeps the noise it gets
 * unsharded (wam_wavedec_noisy == image_base 0) */
int wam_wavedec_noisy_ex(const wam_plan* plan, int64_t n_samples, int64_t images, int channels,
                         const float* x, const float* sigma, uint64_t seed, int64_t sample_base,
                         int64_t image_base, float* coeffs, void* workspace, void* stream);

/* Backward pass of waverec fused with the WAM epilogue (lib/wam_2D.py:116 loss.backward() through
 * ptwt.waverec2, then :227-256 channel mean, |.|, batch-global max): for every image
 * (groups x group_items, channels planes each) the item-major |mean_c| maps (as
 * wam_subband_maps) and band_max[group, band] (caller zero-fills). coeff_grads != NULL also
 * receives the per-channel coefficient gradients (band-major), e.g. for side attributes.
 * WAM_ERR_UNSUPPORTED unless WAM_CAP_ADJOINT_MAPS and channels in {1, 3}. */
int wam_waverec_adjoint_maps(const wam_plan* plan, int64_t groups, int64_t group_items, int channels,
                             const float* grad, float* maps, float* band_max, float* coeff_grads,
                             void* workspace, void* stream);

/* The model hand-off in the explained model's own dtype and layout (lib/wam_2D.py:113-116 with a
 * bf16 channels-last model): wam_waverec_bf16_nhwc is wam_waverec whose reconstruction is written
 * as bf16 images in NHWC order, out [n_alpha * batch / channels, H, W, channels] (plane b = image
 * b / channels, channel b % channels), each value rounded to nearest even exactly as torch's
 * float -> bfloat16 cast; wam_waverec_adjoint_maps_bf16_nhwc is wam_waverec_adjoint_maps over
 * a bf16 NHWC input gradient grad [groups * group_items, H, W, channels] (values widened exactly;
 * no coefficient gradients). Both need WAM_CAP_BF16_NHWC and channels in {1, 3}; no workspace. */
int wam_waverec_bf16_nhwc(const wam_plan* plan, int64_t batch, const float* coeffs, const float* alpha,
                          int n_alpha, int channels, void* out, void* stream);
int wam_waverec_adjoint_maps_bf16_nhwc(const wam_plan* plan, int64_t groups, int64_t group_items, int channels,
                                       const void* grad, float* maps, float* band_max, void* stream);
/* the same for a bf16 gradient in either layout: nhwc != 0 as above, nhwc == 0 planar NCHW
 * [groups * group_items, channels, H, W] (what a model whose first layer's backward ends in a
 * planar op, e.g. a pixel shuffle, hands back) */
int wam_waverec_adjoint_maps_bf16(const wam_plan* plan, int64_t groups, int64_t group_items, int channels, int nhwc,
                                  const void* grad, float* maps, float* band_max, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Live per-launch timing (profiling aid used by bench.py). While enabled every kernel launch is
 * bracketed by hipEventRecord on its stream and logged with its kernel name and ALGORITHMIC
 * bytes; wam_timing_drain synchronises on the recorded events, copies up to max_records
 * (names: 64 chars each) and clears the log. Returns the number of records copied.
 * ---------------------------------------------------------------------------------------------- */
int wam_timing_enable(int on);
/* dst = src (bytes % 16 == 0, 16-B aligned): a streaming copy kernel, the measured HBM ceiling */
int wam_copy(int64_t bytes, const void* src, void* dst, void* stream);
int wam_timing_drain(int max_records, char* names, float* ms, double* bytes);

/* ------------------------------------------------------------------------------------------------
 * SmoothGrad noise (lib/wam_2D.py:390-403, lib/wam_1D.py:311-322, lib/wam_3D.py:565-579)
 * ---------------------------------------------------------------------------------------------- */
/* sigma[i] = fp32(spread) * (max(x_i[0:len]) - min(x_i[0:len])), x_i = x + i*item_stride */
int wam_item_sigma(int64_t items, int64_t item_stride, int64_t len, const float* x, float spread,
                   float* sigma, void* stream);
/* the same sigma as a full-chip split reduction (items x ranges workgroups; the last range of an
 * item to finish combines the partials). ws: wam_item_sigma_ws_bytes(items, len) bytes, 8-byte
 * aligned, zero-filled before its first use with these (items, len); the call leaves it reusable
 * for the same (items, len). */
int64_t wam_item_sigma_ws_bytes(int64_t items, int64_t len);
int wam_item_sigma_ws(int64_t items, int64_t item_stride, int64_t len, const float* x, float spread,
                      float* sigma, void* ws, int64_t ws_bytes, void* stream);

/* out[s, i, e] = x[i, e] + noise  for e < noised_len,  0 for noised_len <= e < item_stride
 * noise = host_noise[s, i, e] if host_noise != NULL (parity mode: the numpy legacy stream), else
 *         sigma[i] * N(0,1) from Philox4x32-10 keyed by (seed), counter (sample_base + s, i, e/4).
 * s ranges over [0, n_samples). */
int wam_noise_add(int64_t n_samples, int64_t items, int64_t item_stride, int64_t noised_len,
                  const float* x, const float* sigma, const float* host_noise, uint64_t seed,
                  int64_t sample_base, float* out, void* stream);
/* the same with the Philox item counter offset by item_base (items of a batch-sharded rank) */
int wam_noise_add_ex(int64_t n_samples, int64_t items, int64_t item_stride, int64_t noised_len,
                     const float* x, const float* sigma, const float* host_noise, uint64_t seed,
                     int64_t sample_base, int64_t item_base, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-subband reduction and accumulation (lib/wam_2D.py:200-264 visualize_grad_wam,
 * :268-341 _reproject_wam, :388-415 SmoothGrad mean, :441-459 IG trapezoid;
 * lib/wam_3D.py:127-166 refactor, :585-587 legacy averaging)
 * ---------------------------------------------------------------------------------------------- */
/* maps[item, band-packed] = | mean over `channels` of coeff_grads |   (numpy float32 mean:
 * ((g0 + g1) + g2 ...) / C);  band_max[group, band] = max over the group's items of maps
 * (atomic; caller zero-fills; NULL: maps only). items = groups * group_items; coeff_grads hold
 * items*channels signals. maps layout: item-major, bands packed with wam_plan_band_offset. */
int wam_subband_maps(const wam_plan* plan, int64_t groups, int64_t group_items, int channels,
                     const float* coeff_grads, float* maps, float* band_max, void* stream);

/* SmoothGrad mosaic accumulation. For each group s in [0, groups) in order and item n:
 *   frame[n, p] += fp64( maps[(s*group_items+n), src[p]] / band_max[s, band[p]] )  (normalize)
 *   frame[n, p] += fp64( maps[...] )                                              (!normalize)
 * src[p] = -1 leaves frame[n, p] unchanged (the reference's zero canvas). frame: [group_items,
 * frame_len] float64. src/band: the mosaic gather map built on the host from the reference's
 * slice-assignment rules (frame geometry lives in the Python layer). */
int wam_frame_accumulate(int64_t groups, int64_t group_items, int64_t frame_len, const int32_t* src,
                         const int32_t* band, const float* maps, int64_t maps_item_len,
                         const float* band_max, int n_bands, int normalize, double* frame,
                         void* stream);

/* wam_frame_accumulate in coefficient order (same sums, bit-identical): dst[k] = the frame pixel
 * of packed coefficient k or -1, cband[k] its band (the inverse of the injective src/band mosaic
 * map, built by the caller: wam_amd/plan.py frame_accumulate). The maps are read as contiguous
 * rows, only the fp64 frame goes through the mosaic. */
int wam_frame_accumulate_coef(int64_t groups, int64_t group_items, int64_t maps_item_len, int64_t frame_len,
                              const int32_t* dst, const int32_t* cband, const float* maps,
                              const float* band_max, int n_bands, int normalize, double* frame, void* stream);

/* Integrated-Gradients mosaic + trapezoid (np.trapz(np.nan_to_num(G), axis=1), dx = 1, fp32).
 * For step k = k0 + s, s in [0, groups):  G = nan_to_num(fp32 mosaic value (normalised));
 *   sequential (weights == NULL): if k > 0: acc += (prev + G) / 2;  prev = G
 *   weighted   (weights != NULL): acc += weights[s] * G     (used when steps are sharded)
 * prev / acc: [group_items, frame_len] fp32. */
int wam_frame_trapz(int64_t groups, int64_t k0, int64_t group_items, int64_t frame_len,
                    const int32_t* src, const int32_t* band, const float* maps, int64_t maps_item_len,
                    const float* band_max, int n_bands, int normalize, const float* weights,
                    float* prev, float* acc, void* stream);

/* wam_frame_trapz in coefficient order (dst / cband as for wam_frame_accumulate_coef): the maps
 * are read as contiguous rows, prev / acc go through the mosaic. Pixels outside the mosaic are not
 * touched -- their G is 0, so with prev == 0 there (zero-initialised, as wam_amd/wam_2D.py passes
 * them) the result is bit-identical to wam_frame_trapz. */
int wam_frame_trapz_coef(int64_t groups, int64_t k0, int64_t group_items, int64_t maps_item_len, int64_t frame_len,
                         const int32_t* dst, const int32_t* cband, const float* maps, const float* band_max,
                         int n_bands, int normalize, const float* weights, float* prev, float* acc, void* stream);

/* 3D cube (lib/wam_3D.py:127-166 refactor; :585-587 legacy averaging; :638 IG trapezoid):
 * value = maps[item, src[p]] with maps = |coeff grads| from wam_subband_maps(channels = 1)
 * (no channel mean, no normalisation). For s in [0, groups) in order:
 * mode 0 (legacy smooth, sequential): acc = (acc + value) / n_total                    (fp32)
 * mode 1 (weighted):                   acc += weights[s] * value
 * mode 2 (IG sequential trapz):        G = nan_to_num(value); if k0+s > 0: acc += (prev+G)/2;
 *                                      prev = G
 * acc / prev: [group_items, cube_len] fp32. */
int wam_cube_accumulate(int64_t groups, int64_t k0, int64_t group_items, int64_t cube_len,
                        const int32_t* src, const float* maps, int64_t maps_item_len, int mode,
                        float n_total, const float* weights, float* prev, float* acc, void* stream);

/* Sum reduction in sample order: acc[e] (+)= src[s*len + e] for s < groups (fp32, sequential);
 * scale != 0: afterwards acc[e] = acc[e] / scale (numpy mean's true_divide). */
int wam_accumulate_f32(int64_t groups, int64_t len, const float* src, float scale, float* acc,
                       void* stream);

/* IG trapezoid over a generic fp32 stream (1D melspec / coefficient gradients):
 * G_s = src[s*len + e]; sequential (weights == NULL) or weighted trapz as in wam_frame_trapz;
 * acc_f64 != NULL accumulates in fp64 (the reference's float64 path_melspecs), else acc_f32. */
int wam_trapz_f32(int64_t groups, int64_t k0, int64_t len, const float* src, const float* weights,
                  float* prev_f32, float* acc_f32, double* prev_f64, double* acc_f64, void* stream);

/* Second moments of the SmoothGrad samples (SmoothGrad-squared, VarGrad). With v the float32 value
 * the matching sum entry adds at an element for sample s (formed by the same operations), every
 * entry below updates, for s in [0, groups) in order,
 *   sum += fp64(v),  sumsq += fp64(v) * fp64(v)     (the product is exact in float64)
 * reading each map value once. sum / sumsq are float64, laid out like the sum entry's accumulator,
 * owned and zeroed by the caller; launches chain (groups 3 then 2 give the bits of one launch of 5).
 * wam_frame_moments(_coef): v of wam_frame_accumulate(_coef), same arguments; sum comes out
 * bit-identical to the frame those entries write, and the two orders give equal bits.
 * wam_cube_moments: v of wam_cube_accumulate (the gathered |g| voxel, 0 where src[p] = -1), plain
 * weights of 1 (not the legacy running average).
 * wam_moments_f32: v = src[s*len + e], element-wise. */
int wam_frame_moments(int64_t groups, int64_t group_items, int64_t frame_len, const int32_t* src,
                      const int32_t* band, const float* maps, int64_t maps_item_len, const float* band_max,
                      int n_bands, int normalize, double* sum, double* sumsq, void* stream);
int wam_frame_moments_coef(int64_t groups, int64_t group_items, int64_t maps_item_len, int64_t frame_len,
                           const int32_t* dst, const int32_t* cband, const float* maps, const float* band_max,
                           int n_bands, int normalize, double* sum, double* sumsq, void* stream);
int wam_cube_moments(int64_t groups, int64_t group_items, int64_t cube_len, const int32_t* src,
                     const float* maps, int64_t maps_item_len, double* sum, double* sumsq, void* stream);
int wam_moments_f32(int64_t groups, int64_t len, const float* src, double* sum, double* sumsq, void* stream);

/* (sum, sumsq) over n >= 1 samples -> out[e], in float64:
 *   kind 0: sum / n                                      (the SmoothGrad mean; sumsq may be NULL)
 *   kind 1: sumsq / n                                    (SmoothGrad-squared; sum may be NULL)
 *   kind 2: max(fma(-m, m, sumsq / n), 0), m = sum / n   (VarGrad: the population variance; NaN
 *           propagates, n = 1 gives exactly 0)
 * written to exactly one of out_f64 / out_f32 (the float64 result rounded once). */
int wam_moments_finish(int64_t len, const double* sum, const double* sumsq, int64_t n, int kind,
                       double* out_f64, float* out_f32, void* stream);

/* .scales side output (lib/wam_2D.py:488-536 reproject_wam): for each item and level j,
 * out[item, j] = sum over the H, V, D quadrants of bilinear (cv2 INTER_LINEAR, half-pixel)
 * upsampling to size x size; with approx, out[item, J] = upsampled approximation corner. The
 * quadrants split at int(size / 2^j); WAM_ERR_INVALID_ARG when size < 2^levels (an empty
 * quadrant: the reference's resize raises on it). */
int wam_reproject_scales(int64_t items, int size, int levels, int approx, const double* avg,
                         double* out, void* stream);

/* BaseWAM2D.scales (lib/wam_2D.py:133-198 disentangle_scales): maps = item-major |channel mean|
 * coefficient-gradient maps of `items` images (wam_subband_maps / wam_waverec_adjoint_maps with one
 * group), band_max = their per-band maxima over the batch. out[item, j] (j < levels, finest
 * first) = (V + D) + H, each band / band_max upsampled to size x size (cv2 INTER_LINEAR on float32,
 * half-pixel centres) in float32, stored as float64; with approx, out[items-1, levels] = the
 * upsampled normalised approximation and out[i < items-1, levels] = 0 (the reference writes only
 * its stale loop index, :194-197). out: [items, levels (+1), size, size] float64. */
int wam_disentangle_scales(const wam_plan* plan, int64_t items, const float* maps, const float* band_max,
                           int approx, int size, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Wavelet-domain insertion / deletion / mu-fidelity (src/evaluation_helpers.py:
 * 361-594 called by Eval2DWAM, src/evaluators.py:553-801). The reference's per-mask CPU loop
 * pywt.wavedec2 -> coeffs_to_array -> arr * mask -> waverec2 -> uint8 -> ToTensor/Normalize
 * becomes: wam_wavedec (mode symmetric) once per image, wam_coeff_masks, wam_waverec of all masks
 * in one launch, wam_quantize_normalize.
 * ---------------------------------------------------------------------------------------------- */
/* generate_masks (:455-505) from a ranking: rank[p] = position of pixel p in the descending
 * importance order; masks [n_iter + 1, len] float32: mask m = 1 where rank < thr(m), thr(0) = 0,
 * thr(m) = m * n_comp, thr(n_iter) = len (deletion != 0: the complement). */
int wam_rank_masks(int64_t n_iter, int64_t n_comp, int64_t len, const int32_t* rank, int deletion,
                   float* masks, void* stream);
/* arr * masks[m] in pywt.coeffs_to_array's layout: coefficient k (band-major item offset) of each
 * of `items` planes sits at array position pos[k] (< mask_len). out: band-major coefficients of
 * n_masks * items planes, plane (m, i) = m * items + i. */
int wam_coeff_masks(const wam_plan* plan, int64_t items, const float* coeffs, const int32_t* pos,
                    int64_t n_masks, int64_t mask_len, const float* masks, float* out, void* stream);
/* per image (channels x plane floats): normalize_data (min-max, float32), (v * 255) -> uint8
 * (truncation), / 255, (- mean[c]) / std[c] (torchvision ToTensor + Normalize); mean / std are
 * HOST arrays of `channels` (<= 4) values. */
int wam_quantize_normalize(int64_t images, int channels, int64_t plane, const float* rec, const float* mean,
                           const float* std, float* out, void* stream);
/* The same quantisation followed by torchvision Resize((out_h, out_w)) on the PIL image (Pillow's
 * 8-bit BILINEAR resample) and ToTensor + Normalize, for reconstructions that are not 224 x 224:
 * Eval2DWAM's default transform (src/evaluators.py:593-598) on e.g. 256^2 inputs. Replaces the
 * reference's per-image PIL path (src/evaluators.py:631-633). rec [images, channels, in_h, in_w]
 * float32 -> out [images, channels, out_h, out_w] float32. The resample tables are Pillow's
 * (precompute_coeffs + normalize_coeffs_8bpc, wam_amd/evaluation.py pil_bilinear_coeffs): per
 * output column xx bounds_h[2 xx] = first source column, bounds_h[2 xx + 1] = count, kk_h[xx *
 * ksize_h + k] = 22-bit fixed-point weights (device int32); likewise vertically with the bounds
 * relative to source row y0. bounds_h == NULL: the width is unchanged (no horizontal pass; y0 /
 * tmp_h ignored, bounds_v absolute); bounds_v == NULL: the height is unchanged. tmp_h = source
 * rows the vertical pass reads (y0 .. y0 + tmp_h - 1). scratch: images * channels * (in_h * in_w +
 * tmp_h * out_w) bytes. Bit-identical to PIL.Image.resize((out_w, out_h), BILINEAR). */
int wam_quantize_resize_normalize(int64_t images, int channels, int in_h, int in_w, const float* rec, int out_h,
                                  int out_w, int ksize_h, const int32_t* bounds_h, const int32_t* kk_h, int ksize_v,
                                  const int32_t* bounds_v, const int32_t* kk_v, int y0, int tmp_h, const float* mean,
                                  const float* std, uint8_t* scratch, float* out, void* stream);
/* scipy.ndimage.gaussian_filter of items h x w float64 maps, mode 'reflect' (half-sample
 * symmetric): weights[0..radius] = the symmetric 1-D kernel (host), axis 0 then axis 1, scipy's
 * accumulation order; tmp: items * h * w doubles of scratch. */
int wam_gaussian_filter2d(int64_t items, int h, int w, const double* weights, int radius, const double* in,
                          double* tmp, double* out, void* stream);
/* The same filter on items of d x h x w float64 volumes (Eval3DWAM.mu_fidelity): three 1-D passes over
 * axes 0, 1, 2 of every item with the pass of the 2D entry -- x0 * w[0], then acc + (x[-j] + x[+j]) * w[j]
 * for j = radius .. 1, every product and sum rounded, no fma -- which is scipy.ndimage.gaussian_filter's
 * float64 result bit for bit (mode 'reflect', any number of reflections: an extent may be smaller than
 * the radius). Pass order in -> out, out -> tmp, tmp -> out: `in` is left untouched, tmp and out hold
 * items * d * h * w doubles each and are distinct from `in` and from each other. radius 0 copies `in`
 * through the three passes (x * w[0] each). WAM_ERR_INVALID_ARG: items < 0, an extent < 1, d * h * w >
 * INT32_MAX, radius < 0 or > 64, a NULL weights, in, tmp or out. items == 0 returns WAM_OK. */
int wam_gaussian_filter3d(int64_t items, int d, int h, int w, const double* weights, int radius,
                          const double* in, double* tmp, double* out, void* stream);
/* out[m, p] = grid[m, cell[p]]  (nearest-neighbour zoom through a precomputed cell map) */
int wam_upsample_masks(int64_t n_masks, int64_t grid_len, const float* grid, int64_t out_len,
                       const int32_t* cell, float* out, void* stream);
/* sum_importance (:361-393): out[m] = sum_p wam[p] * grid[m, cell[p]] (float64) */
int wam_masked_sums(int64_t n_masks, int64_t len, const double* wam, int64_t grid_len, const float* grid,
                    const int32_t* cell, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Audio insertion / deletion / faithfulness of spectra / input fidelity (Eval1DWAM,
 * src/evaluators.py:39-306). The reference's per-clip CPU loop (masks on the host, coeff * mask per
 * band, float64 pywt.waverec of n_iter + 1 sets, numpy wf / wf.max()) becomes: wam_wavedec (mode
 * reflect) once per group of clips, wam_rank_mask_coeffs, one wam_waverec, wam_peak_normalize, the
 * mel front-end. The masks themselves are never stored.
 * The selection rule shared by the two rank-mask entries, for mask m = 0 .. n_iter of a set whose
 * ranking has rank_len slots: thr(0) = 0; thr(m) = min(m * n_comp, rank_len) for 0 < m < n_iter;
 * thr(n_iter) = rank_len. A value whose mask slot is p is kept by mask m when
 * (rank[s, p] < thr(m)) != (deletion != 0). A kept value is multiplied by 1.0f, a dropped one by
 * 0.0f (so a dropped negative value is -0.0f and a dropped NaN stays NaN).
 * ---------------------------------------------------------------------------------------------- */
/* Ranking to masked coefficients. plan: a 1D plan (WAM_ERR_UNSUPPORTED otherwise) with K =
 * wam_plan_coeff_numel values per item. coeffs: band-major coefficients of `sets` items, as
 * wam_wavedec writes them (band b of item s starts at sets * off[b] + s * n_b, off[b] =
 * wam_plan_band_offset, n_b the band length). rank [sets, rank_len] int32 (device): rank[s, p] = the
 * position of mask slot p of set s in the descending importance order. pos [K] int32 (device), shared
 * by all sets: pos[k] = the mask slot of the coefficient at per-item offset k (k = off[b] + e for
 * element e of band b), in [0, rank_len), or -1 for the reference's pad column; any other value is
 * read as -1. A pad-column coefficient is kept by every mask under insertion and dropped by every
 * mask under deletion. out: band-major coefficients of sets * (n_iter + 1) items, item (s, m) =
 * s * (n_iter + 1) + m, i.e. out[sets * (n_iter + 1) * off[b] + (s * (n_iter + 1) + m) * n_b + e] =
 * coeffs[sets * off[b] + s * n_b + e] * keep: the buffer wam_waverec reads with batch =
 * sets * (n_iter + 1). n_iter >= 1, n_comp >= 0, rank_len >= 1. */
int wam_rank_mask_coeffs(const wam_plan* plan, int64_t sets, const float* coeffs, const int32_t* rank,
                         int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion,
                         float* out, void* stream);
/* The same selection on flat rows with the identity slot map (the mel target): src [sets, len]
 * float32, rank [sets, len] int32, out [sets, n_iter + 1, len] float32:
 * out[s, m, i] = src[s, i] * keep(rank[s, i], m) with rank_len = len. */
int wam_rank_mask_rows(int64_t sets, int64_t len, const float* src, const int32_t* rank, int64_t n_iter,
                       int64_t n_comp, int deletion, float* out, void* stream);
/* Peak normalisation of `rows` rows of `len` float32 (numpy's wf / wf.max() per reconstruction):
 * mx[r] = the signed maximum of row r (not of its absolute values); out[r, i] = in[r, i] / mx[r] in
 * IEEE fp32 division (correctly rounded, no reciprocal multiply); silent[r] (int32, device, may be
 * NULL) = 1 when mx[r] == 0 and 0 otherwise. A silent row divides by zero as IEEE does: 0 / 0 = NaN,
 * a negative value / 0 = -inf. With zero_silent != 0 a silent row is copied unchanged instead. out
 * may be `in` (in place). Inputs are finite: a NaN input is ignored by the maximum and an all-NaN
 * row has mx = -inf; neither is part of the contract. */
int wam_peak_normalize(int64_t rows, int64_t len, const float* in, float* out, int32_t* silent, int zero_silent,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ranked synthesis: the n_iter + 1 masked reconstructions of every item straight from a ranking, in one
 * call. wam_waverec_ranked serves 3D plans only, wam_waverec2_ranked 2D plans and wam_waverec1_ranked 1D
 * plans; the three share one implementation and the contract of this section, and each block below states
 * its layout, its route 1 and its differences only.
 * Selection. The rule, the layout of coeffs, rank and pos and the pad rule are exactly those of
 * wam_rank_mask_coeffs: thr(0) = 0, thr(m) = min(m * n_comp, rank_len), thr(n_iter) = rank_len; mask m of
 * an item keeps the coefficient at per-item offset k when (rank[row, pos[k]] < thr(m)) != (deletion != 0),
 * row being the item's rank row; a pos[k] of -1 or outside [0, rank_len) reads as rank -1 (kept by every
 * mask under insertion, dropped by every mask under deletion); two coefficients may share a slot; a kept
 * value is multiplied by 1.0f and a dropped one by 0.0f (a dropped negative value is -0.0f, a dropped NaN
 * stays NaN), the approximation like any other band. coeffs: band-major coefficients as wam_wavedec
 * writes them; rank [rows, rank_len] int32 (device); pos [K] int32 (device), K = wam_plan_coeff_numel,
 * shared by all items. Output item (item, m) = wam_waverec of the item masked by m.
 * Routes. Two routes compute the output, bit-identical to each other:
 *   route 0: the masked sets are written band-major into the workspace (what wam_rank_mask_coeffs
 *     writes, over all bands of the plan) and the plan's wam_waverec reads them, whatever route its
 *     synthesis takes: every plan of the entry's dimension, any alignment of coeffs, rank, pos and out.
 *     Workspace: the (n_iter + 1) * K floats of every item, rounded up to 16 bytes, followed by
 *     wam_plan_workspace_bytes(plan, output items);
 *   route 1: a fused kernel applies the threshold as the synthesis loads its coefficients; no masked
 *     coefficient is stored. The plans it serves and the pointers it takes are stated per dimension;
 *   route -1: the plan's own route, which wam_waverec*_ranked_route returns: 1 wherever route 1 serves the
 *     plan, else 0. The route queries work on host-only plans and are negative for a NULL plan or a plan
 *     of another dimension.
 * Fallback. Forcing route 1 on a plan it does not serve returns WAM_ERR_UNSUPPORTED and launches nothing;
 * forcing it with pointers it cannot take returns WAM_ERR_UNSUPPORTED. With route -1 a call that route 1
 * cannot take runs route 0 in the same workspace.
 * Errors. A plan of another dimension: WAM_ERR_UNSUPPORTED. WAM_ERR_INVALID_ARG: a NULL plan, coeffs, rank,
 * pos or out, a negative item count, rank_len < 1 or > INT32_MAX, n_iter < 1, n_comp < 0, a host-only
 * plan, another route value, more than 65535 * 16 masks on route 0, and a NULL or misaligned (16 bytes)
 * workspace where the route reads one; nothing is launched then. An item count of 0 returns WAM_OK, with
 * any workspace. The *_workspace_bytes queries return 0 for invalid arguments.
 * ---------------------------------------------------------------------------------------------- */

/* ---- 3D: insertion / deletion of voxel WAMs (Eval3DWAM; an addition, the reference evaluates no
 * volumes). One rank row per set. out [sets * (n_iter + 1), *rec_shape] float32: volume s * (n_iter + 1) + m.
 *   route 0 expands over the 1 + 7 * levels bands;
 *   route 1: 3D Haar plans with levels <= 2 and dimensions divisible by 2^levels whose wam_waverec runs
 *     the fused block kernel (not WAM_PLAN_GENERIC); no workspace is read. It needs out 16-byte and
 *     coeffs and pos 8-byte aligned. */
/* the route a plan takes by itself: 1 = the fused Haar kernel where it applies (the faster one there,
 * profiles/eval3d_kbench.txt) */
int    wam_waverec_ranked_route(const wam_plan* plan);
/* bytes of workspace wam_waverec_ranked needs on `route`: route 1 none; route 0 as above; -1 (the plan's
 * own) the own route's size, 0 where it is route 1 */
size_t wam_waverec_ranked_workspace_bytes(const wam_plan* plan, int64_t sets, int64_t n_iter, int route);
/* workspace (device, 16-byte aligned): at least wam_waverec_ranked_workspace_bytes(plan, sets, n_iter, 0)
 * bytes on route 0, not read on route 1 (may be NULL). With route -1 a call whose pointers route 1 cannot
 * take runs route 0 when a workspace is given, and returns WAM_ERR_UNSUPPORTED without one. A NULL or
 * misaligned workspace is WAM_ERR_INVALID_ARG on route 0 only. More than 65535 * 16 masks is
 * WAM_ERR_INVALID_ARG on either route. */
int    wam_waverec_ranked(const wam_plan* plan, int64_t sets, const float* coeffs, const int32_t* rank,
                          int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion,
                          int route /* -1: the plan's own */, float* out /* [sets*(n_iter+1), *rec_shape] */,
                          void* workspace, void* stream);

/* ---- 2D: insertion / deletion of image WAMs by ranking (Eval2DWAM with mask_layout="mosaic"). The
 * items are images * channels planes, channels in 1..4; coeffs holds plane (n, c) = n * channels + c
 * (wam_threshold_mask_coeffs's layout); rank [images, rank_len]: one ranking per image shared by its
 * channels. out [images, n_iter + 1, channels, rec_h, rec_w] float32: image n, mask m is a contiguous
 * [channels, rec_h, rec_w] block.
 *   route 0 expands over the 1 + 3 * levels bands into planes (n, m, c);
 *   route 1: plans whose wam_waverec runs the plane-resident synthesis (filters up to 8 taps whose
 *     levels fit its LDS, not WAM_PLAN_GENERIC / WAM_PLAN_NO_PLANE): a pre-pass writes the ranking in
 *     coefficient order once per image (images * K int32 of workspace), and the synthesis applies the
 *     threshold as it loads its coefficient rows. It needs out 8-byte aligned (its pixel pairs are
 *     8-byte stores); coeffs, rank and pos need only their natural 4. */
/* the route a plan takes by itself: 1 = the fused plane-resident kernel (only where it measured faster,
 * profiles/eval2d_kbench.txt) */
int    wam_waverec2_ranked_route(const wam_plan* plan);
/* bytes of workspace wam_waverec2_ranked needs on `route`: route 1 the rank table, images * K int32
 * rounded up to 16 bytes; route 0 as above over images * channels planes; -1 (the plan's own) route 0's
 * size, which is the fallback's and holds route 1's table too. 0 also for channels outside 1..4. */
size_t wam_waverec2_ranked_workspace_bytes(const wam_plan* plan, int64_t images, int channels, int64_t n_iter,
                                           int route);
/* workspace (device, 16-byte aligned): at least wam_waverec2_ranked_workspace_bytes(plan, images,
 * channels, n_iter, route) bytes on every route; a NULL or misaligned one is WAM_ERR_INVALID_ARG. Also
 * WAM_ERR_INVALID_ARG: channels outside 1..4, and more than INT32_MAX (plane, mask) pairs on route 1 (the
 * one error found after a launch: the rank table is already written then). */
int    wam_waverec2_ranked(const wam_plan* plan, int64_t images, int channels, const float* coeffs,
                           const int32_t* rank, int64_t rank_len, const int32_t* pos, int64_t n_iter,
                           int64_t n_comp, int deletion, int route /* -1: the plan's own */,
                           float* out /* [images, n_iter+1, channels, rec_h, rec_w] */, void* workspace,
                           void* stream);

/* ---- 1D: insertion / deletion of audio WAMs with every coefficient ranked by its own gradient
 * (Eval1DWAM with mask_layout="coeffs"): the reconstructions and their peak values in one call, then the
 * division (wam_peak_divide). One rank row per set. out [sets * (n_iter + 1), rec_len] float32, rec_len =
 * wam_plan_rec_shape: row s * (n_iter + 1) + m. row_max [sets * (n_iter + 1)] float32 (device, may be
 * NULL): row_max[r] = the signed maximum of out row r over rec_len, bit-equal to the maximum
 * wam_peak_normalize reduces, a zero maximum written as +0.0f; inputs are finite, as in
 * wam_peak_normalize's contract. The two routes are bit-identical in out and in row_max.
 *   route 0 expands over the 1 + levels bands, and a max-only reduction pass fills row_max when it is
 *     given;
 *   route 1: plans whose wam_waverec runs the persistent fused tile kernel on every tile (filters up to
 *     20 taps, levels <= 8, the register and LDS footprint of that kernel, a non-periodic mode, not
 *     WAM_PLAN_GENERIC; an (L, levels) whose ranked kernel would spill registers is excluded too --
 *     none is today): a pre-pass writes the ranking in coefficient order once per set (sets * K int32 of
 *     workspace), and the synthesis applies the threshold as it stages its coefficients; each workgroup
 *     adds the maximum of the outputs it wrote to row_max with one atomic (row_max is set to -inf first;
 *     the maximum does not depend on the order). Any alignment. */
/* the route a plan takes by itself: 1 = the fused tile kernel wherever it applies (its slowest round beat
 * route 0's fastest at every filter length from 2 to 20 taps, profiles/eval1d_ranked_kbench.txt) */
int    wam_waverec1_ranked_route(const wam_plan* plan);
/* bytes of workspace wam_waverec1_ranked needs on `route`: route 1 the rank table, sets * K int32 rounded
 * up to 16 bytes; route 0 as above; -1 (the plan's own) route 0's size, which is the fallback's and holds
 * route 1's table too */
size_t wam_waverec1_ranked_workspace_bytes(const wam_plan* plan, int64_t sets, int64_t n_iter, int route);
/* workspace (device, 16-byte aligned): at least wam_waverec1_ranked_workspace_bytes(plan, sets, n_iter,
 * route) bytes on every route; a NULL or misaligned one is WAM_ERR_INVALID_ARG. Also WAM_ERR_INVALID_ARG,
 * on either route and before any launch: more than 65535 * 16 masks, more than INT32_MAX output rows. */
int    wam_waverec1_ranked(const wam_plan* plan, int64_t sets, const float* coeffs, const int32_t* rank,
                           int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp, int deletion,
                           int route /* -1: the plan's own */, float* out /* [sets*(n_iter+1), rec_len] */,
                           float* row_max /* [sets*(n_iter+1)] or NULL */, void* workspace, void* stream);
/* The second half of wam_peak_normalize, given the maxima (wam_waverec1_ranked's row_max): out[r, i] =
 * in[r, i] / row_max[r] in IEEE fp32 division (correctly rounded, no reciprocal multiply); silent[r]
 * (int32, device, may be NULL) = (row_max[r] == 0). A silent row divides by zero as IEEE does; with
 * zero_silent != 0 it is copied unchanged instead. out may be `in` (in place). Each row is read once and
 * written once, with 16-byte accesses when len is a multiple of 4 and in and out are 16-byte aligned.
 * WAM_ERR_INVALID_ARG: rows < 0 or > INT32_MAX, len < 1, a NULL in, row_max or out, more than INT32_MAX
 * spans of 4096 elements over all rows. rows == 0 returns WAM_OK. */
int    wam_peak_divide(int64_t rows, int64_t len, const float* in, const float* row_max, float* out,
                       int32_t* silent, int zero_silent, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cell-mask synthesis: the reconstructions of every volume under n_masks float-valued superpixel masks,
 * in one call (Eval3DWAM.mu_fidelity; an addition, the reference evaluates no volumes). 3D plans only.
 * coeffs: band-major coefficients of `sets` volumes as wam_wavedec writes them. slot [K] int32 (device),
 * K = wam_plan_coeff_numel, shared by all sets: slot[k] = the grid cell of the coefficient at per-item
 * offset k. grid [sets, n_masks, grid_len] float32 (device): every set has its own masks. Output volume
 * s * n_masks + m is wam_waverec of set s with every coefficient -- the approximation like any other
 * band -- multiplied by f = grid[(s * n_masks + m) * grid_len + slot[k]] when 0 <= slot[k] < grid_len and
 * by f = 1.0f otherwise, so that any slot value is memory-safe. The product is one fp32 multiply c * f,
 * not a select: a NaN coefficient times 0 stays NaN, a negative one times 0 is -0.0f. The synthesis
 * after it is wam_waverec's with scale 1.
 * Routes, as in the ranked section above, bit-identical to each other:
 *   route 0: the masked sets are written band-major into the workspace (over the 1 + 7 * levels bands)
 *     and the plan's wam_waverec reads them: every 3D plan, any alignment. Workspace: sets * n_masks * K
 *     floats rounded up to 16 bytes, followed by wam_plan_workspace_bytes(plan, sets * n_masks);
 *   route 1: 3D Haar plans with levels <= 2 and dimensions divisible by 2^levels whose wam_waverec runs
 *     the fused block kernel (not WAM_PLAN_GENERIC). A workgroup serves one set and a chunk of up to 16
 *     masks: a thread loads its block's coefficients and slots once and, per mask, gathers the factors
 *     from the mask's grid row, multiplies, inverts the levels and stores the block; no masked coefficient
 *     is stored and no workspace is read. It takes grid_len <= 65535 (a thread keeps its cells in 16 bits;
 *     the default 8^3 grid has 512; measured at 64 and 512 cells only), at most 65535 sets, out 16-byte and
 *     coeffs and slot 8-byte aligned. The gather reads global memory through the caches; staging the rows
 *     in LDS first measured 3 to 4 % slower at 128^3 and is kept as a build option only (it would bound
 *     grid_len by 1023);
 *   route -1: the plan's own route, which wam_waverec_cells_route returns.
 * Forcing route 1 on a plan, a grid_len or pointers it cannot take returns WAM_ERR_UNSUPPORTED and
 * launches nothing. With route -1 such a call runs route 0 when a workspace is given and returns
 * WAM_ERR_UNSUPPORTED without one.
 * Errors. A plan of another dimension: WAM_ERR_UNSUPPORTED. WAM_ERR_INVALID_ARG: a NULL plan, coeffs,
 * slot, grid or out, sets < 0, n_masks < 1, grid_len < 1, a host-only plan, another route value, more
 * than 65535 * 16 masks, and a NULL or misaligned (16 bytes) workspace on route 0; nothing is launched
 * then. sets == 0 returns WAM_OK.
 * ---------------------------------------------------------------------------------------------- */
/* the route a plan takes by itself: 1 = the fused Haar kernel wherever it applies, else 0. Route 1 was the
 * faster one at every geometry of profiles/eval3d_cells_kbench.txt, its slowest round against route 0's
 * fastest: Haar J=2 at 128^3 with 1 and 4 volumes x 128 masks on an 8^3 grid (about 0.19 against 0.63 -
 * 0.67 ms and 0.72 against 2.3 ms), Haar J=1 and J=2 at 16^3 with 16 volumes x 128 masks on a 4^3 grid
 * (about 11 against 34 us and 13 against 32 us). Works on host-only plans; negative for a NULL plan
 * (-WAM_ERR_INVALID_ARG) or a plan of another dimension (-WAM_ERR_UNSUPPORTED). */
int    wam_waverec_cells_route(const wam_plan* plan);
/* bytes of workspace wam_waverec_cells needs on `route`: route 1 none; route 0 as above; -1 the own
 * route's size (0 where it is route 1: size it with route 0 when grid_len may exceed route 1's limit).
 * 0 for invalid arguments. Works on host-only plans. */
size_t wam_waverec_cells_workspace_bytes(const wam_plan* plan, int64_t sets, int64_t n_masks, int route);
int    wam_waverec_cells(const wam_plan* plan, int64_t sets, const float* coeffs, const int32_t* slot,
                         int64_t n_masks, int64_t grid_len, const float* grid, int route /* -1: the plan's own */,
                         float* out /* [sets * n_masks, *rec_shape] */, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * WAMAnalyzer2D (src/analyzers.py:16-203, src/analyzers_helpers.py:6-134): necessary components
 * (quantile thresholds on the WAM map) and scale isolation (one mask per level). The reference's
 * per-image, per-quantile CPU loop (3 x pywt.wavedec2 -> coeffs_to_array -> arr * (grad_wam >= t) ->
 * waverec2, then ((x - mn) / mx - mn) * 255 -> uint8 -> PIL -> transform) becomes: wam_wavedec (mode
 * symmetric) once for all images, wam_threshold_mask_coeffs, one wam_waverec,
 * wam_quantize_normalize_ex. The masks themselves are never stored.
 * ---------------------------------------------------------------------------------------------- */
/* Value thresholds to masked coefficients. plan: a 2D plan (WAM_ERR_UNSUPPORTED otherwise) with K =
 * wam_plan_coeff_numel values per plane. coeffs: band-major coefficients of images * channels planes
 * as wam_wavedec writes them, plane (n, c) = n * channels + c (band b of plane i starts at
 * images * channels * off[b] + i * n_b, off[b] = wam_plan_band_offset, n_b the band's element count).
 * pos [K] int32 (device), shared by all planes: pos[k] = the row-major position, in a size x size
 * array, of the coefficient at per-plane offset k (pywt.coeffs_to_array's layout). wam [images,
 * size * size] float64 (device): the map of each image. thr (device, float64): the n_thr thresholds
 * of image n are thr[n * thr_stride + q], q = 0 .. n_thr - 1 (thr_stride >= n_thr).
 * For coefficient k of plane (n, c) and threshold q, with p = pos[k] and v = wam[n, p]:
 *   level_mode == 0: keep = strict ? v > thr[n, q] : v >= thr[n, q], compared in float64 (a NaN v
 *     is never kept);
 *   level_mode != 0: threshold q is level entry q of compute_levelized_masks, n_thr = levels + 1 <=
 *     17, edges (HOST int32 [n_thr], read during the call) = int(size / 2^j), j = 0 .. levels. With
 *     (r, c) = (p / size, p % size) and m = max(r, c), entry q < levels is the region edges[q + 1] <=
 *     m < edges[q] (the three blocks [s:e, s:e], [s:e, :s], [:s, s:e]) and entry `levels` the region
 *     m < edges[levels]; v is replaced by 0.0 when p lies outside entry q's region, then compared as
 *     above.
 * A position outside [0, size * size) is kept by no threshold. out: band-major coefficients of
 * images * n_thr * channels planes, plane (n, q, c) = (n * n_thr + q) * channels + c:
 *   out[images * n_thr * channels * off[b] + ((n * n_thr + q) * channels + c) * n_b + e] =
 *   coeffs[images * channels * off[b] + (n * channels + c) * n_b + e] * (keep ? 1.0f : 0.0f)
 * (a dropped negative value is -0.0f, a dropped NaN stays NaN, as numpy's arr * mask): the buffer
 * wam_waverec reads with batch = images * n_thr * channels. images <= 0, n_thr <= 0 or thr_stride <
 * n_thr: WAM_ERR_INVALID_ARG. That size * size equals the array size of pos is the caller's check. */
int wam_threshold_mask_coeffs(const wam_plan* plan, int64_t images, int channels, const float* coeffs,
                              const int32_t* pos, int size, const double* wam, int64_t n_thr, const double* thr,
                              int64_t thr_stride, int level_mode, const int32_t* edges, int strict, float* out,
                              void* stream);
/* Quantisation of `images` reconstructions (channels <= 4 planes of `plane` floats each), mn / mx =
 * the minimum / maximum over all channels of the image, every operation an IEEE float32
 * round-to-nearest one in the order written:
 *   rule 0: s = ((x - mn) / (mx - mn)) * 255; q = 0 when s is NaN, else s truncated (s is in
 *     [0, 255]): wam_quantize_normalize's rule, `out` bit-identical to it;
 *   rule 1: s = (((x - mn) / mx) - mn) * 255 (src/analyzers.py:155, the reference's precedence); q =
 *     numpy's float32 -> uint8 cast on x86: s truncated toward zero to int32, the low 8 bits kept
 *     (-3.7 -> 253, 300.7 -> 44, 1000.3 -> 232); q = 0 when s is NaN, infinite or |s| >= 2^31.
 * u8 (may be NULL): q as bytes, planar [images, channels, plane]. out (may be NULL; not both):
 * (q / 255 - mean[c]) / std[c] as float32 [images, channels, plane]; mean / std are HOST arrays of
 * `channels` values (needed only with out). */
int wam_quantize_normalize_ex(int64_t images, int channels, int64_t plane, const float* rec, int rule,
                              const float* mean, const float* std, uint8_t* u8, float* out, void* stream);
/* wam_quantize_resize_normalize with the quantisation rule of wam_quantize_normalize_ex in front
 * (rule 0: bit-identical to it); every other argument as there. */
int wam_quantize_resize_normalize_ex(int64_t images, int channels, int in_h, int in_w, const float* rec, int rule,
                                     int out_h, int out_w, int ksize_h, const int32_t* bounds_h, const int32_t* kk_h,
                                     int ksize_v, const int32_t* bounds_v, const int32_t* kk_v, int y0, int tmp_h,
                                     const float* mean, const float* std, uint8_t* scratch, float* out,
                                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pixel-domain baselines (EvalImageBaselines, src/evaluators.py:805-1180; GradCAM, GradCAMPlusPlus,
 * SmoothGrad, src/evaluation_helpers.py:72-320). The reference's per-image, per-mask CPU loop
 * (generate_masks -> masks[i, :, :, None] * img -> normalize_data -> uint8 -> PIL -> transform) and its
 * per-channel Grad-CAM loop become one ranking-to-model-input pass, one superpixel-to-model-input pass
 * and one workgroup per CAM. The masks themselves are never stored.
 * The two mask entries share their outputs. For masked image i (channels <= 4 planes of `plane`
 * floats, v[c, p] below), with mn / mx the minimum / maximum of v over all channels of the image:
 *   masked (float32): v itself;
 *   u8: q = rule 0 of wam_quantize_normalize_ex on v (s = ((v - mn) / (mx - mn)) * 255, every operation
 *       an IEEE float32 one in that order; q = 0 when s is NaN -- the image whose pixels are all equal --
 *       else s truncated);
 *   out (float32): (q / 255 - mean[c]) / std[c], bit-identical to wam_quantize_normalize_ex(rule 0) applied
 *       to `masked`; mean / std are HOST arrays of `channels` values (needed only with out).
 * Each is laid out [images, channels, plane], may be NULL, and at least one is not. Inputs are finite.
 * ---------------------------------------------------------------------------------------------- */
/* Ranking to the model inputs of insertion / deletion. img [sets, channels, plane] float32; rank
 * [sets, plane] int32 (device): rank[s, p] = the position of pixel p of set s in the descending
 * importance order, in [0, plane). The selection rule is the one of the two rank-mask entries above
 * with rank_len = plane: thr(0) = 0, thr(m) = min(m * n_comp, plane) for 0 < m < n_iter, thr(n_iter) =
 * plane; mask m keeps pixel p when (rank[s, p] < thr(m)) != (deletion != 0). Image (s, m) =
 * s * (n_iter + 1) + m has v[c, p] = img[s, c, p] * (keep ? 1.0f : 0.0f) (a dropped negative pixel is
 * -0.0f). ws (device, 4-byte aligned): wam_rank_mask_pixels_ws_bytes(sets, n_iter) = 8 * sets *
 * ((n_iter + 1) + 32 * (n_iter + 2)) bytes, written by the call and needing no initialisation (the
 * extrema of every image, found from one pass over each set -- a pixel enters the kept set at one mask
 * and stays --, and the tables of the up to 32 workgroups that share that pass). sets <= 65535,
 * n_iter >= 1, n_comp >= 0; n_iter > 4096: WAM_ERR_UNSUPPORTED (a workgroup's extrema table is held
 * in LDS). 16-byte stores when plane % 4 == 0
 * and img, rank, masked and out are 16-byte (u8: 4-byte) aligned, scalar ones otherwise; the values are
 * the same. */
int64_t wam_rank_mask_pixels_ws_bytes(int64_t sets, int64_t n_iter);
int wam_rank_mask_pixels(int64_t sets, int channels, int64_t plane, const float* img, const int32_t* rank,
                         int64_t n_iter, int64_t n_comp, int deletion, const float* mean, const float* std,
                         float* masked, uint8_t* u8, float* out, void* ws, void* stream);
/* mu-fidelity's superpixel masks on one image. img [channels, plane] float32; grid [n_masks, grid_len]
 * float32 (device); cell [plane] int32 (device): the grid cell of every pixel (scipy.ndimage.zoom,
 * order 0, as for wam_upsample_masks). Image m has v[c, p] = grid[m, cell[p]] * img[c, p], one float32
 * multiply; a cell outside [0, grid_len) multiplies by 0.0f. */
int wam_cell_mask_pixels(int channels, int64_t plane, const float* img, int64_t n_masks, int64_t grid_len,
                         const float* grid, const int32_t* cell, const float* mean, const float* std, float* masked,
                         uint8_t* u8, float* out, void* stream);
/* Grad-CAM (plus_plus == 0) and Grad-CAM++ as the reference computes them. act, grad [images, K, h, w]
 * float32: the target layer's output and the gradient of the class score with respect to it. Per image:
 *   w_k = mean over h x w of grad_k;  plus_plus != 0: w_k = sum(max(grad_k, 0) * act_k) / (sum(act_k) + 1e-8)
 *   (the reference's formula, not the paper's);
 *   cam = max(sum_k w_k * act_k, 0);  cam -= min(cam);  cam /= max(cam)  (IEEE division: a CAM that is
 *   nowhere positive is 0 / 0, and the whole map is NaN, as in the reference);
 *   out [images, out_h, out_w] float32 = torch's bilinear resize with align_corners=False: source
 *   coordinate scale * (dst + 0.5) - 0.5 in float32 with scale = (float)in / out, clamped at 0.
 * The sums, the normalisation and the interpolation are taken in float64 and rounded to float32 once
 * (the reference accumulates K float32 planes in channel order). One workgroup per image; 8 * (K + h * w
 * + 1040) bytes of LDS, WAM_ERR_UNSUPPORTED above 160 KiB. */
int wam_cam_maps(int64_t images, int64_t K, int h, int w, const float* act, const float* grad, int plus_plus,
                 int out_h, int out_w, float* out, void* stream);
/* The same maps without the LDS bound: any K >= 1 and any h * w <= INT32_MAX, the shapes wam_cam_maps
 * accepts included (full-resolution layers of audio CNNs: 157 x 128 and 431 x 128 mel cells; layer1 of
 * an image ResNet from 640 x 640 inputs up). The contract of the values is the one above, word for word
 * (float64 sums, normalisation and interpolation, one rounding to float32, the all-NaN map); the order of
 * the float64 sums differs from wam_cam_maps, so the two agree to rounding of the float32 result, not in
 * bits. Three launches in stream order: per (image, channel) the weight sums of S = min(64, ceil(h * w /
 * 1024)) splits of the plane, one wave each; per tile of 1024 pixels the weighted sum over k ascending
 * (the splits combined in split order), ReLU, the float64 plane and the tile's extrema; the resize, which
 * reads the plane back. ws (device, 8-byte aligned, written by the call, no initialisation needed):
 * wam_cam_maps_tiled_ws_bytes(images, K, h, w) = 8 * images * (2 * K * S + h * w + 2 * T) bytes with
 * T = ceil(h * w / 1024) (the partial sums, the plane, the tile extrema); negative for invalid arguments.
 * No floating-point atomics: two calls return the same bits. 16-byte loads when h * w % 4 == 0 and act
 * and grad are 16-byte aligned, scalar ones otherwise; the values are the same. Argument errors as for
 * wam_cam_maps, and WAM_ERR_INVALID_ARG for a NULL, misaligned or short ws; images == 0 returns WAM_OK
 * before ws is looked at. */
int64_t wam_cam_maps_tiled_ws_bytes(int64_t images, int64_t K, int h, int w);
int wam_cam_maps_tiled(int64_t images, int64_t K, int h, int w, const float* act, const float* grad,
                       int plus_plus, int out_h, int out_w, float* out, void* ws, int64_t ws_bytes, void* stream);
/* The channel mean the gradient methods end in. g [items, channels, plane] float32; t_c = g[n, c, p],
 * times mult[n, c, p] when mult != NULL (same shape), then its absolute value when absolute != 0;
 * m = ((t_0 + t_1) + ...) / channels in float32, sequential (numpy's order for a short axis).
 * out_f32 [items, plane] = m and / or acc_f64 [items, plane] += (double)m; at least one is not NULL. */
int wam_channel_mean(int64_t items, int channels, int64_t plane, const float* g, const float* mult, int absolute,
                     float* out_f32, double* acc_f64, void* stream);

/* WaveletAttribution3D.visualize (lib/wam_3D.py:662-719): cube [items, S, S, S]
 * float32 (the |grad| cube of smooth / IG) -> out [items, levels + 2, S, S, S] float32: per level
 * the block (approximation corner, or add + ada + add + daa + dad + dda of the detail shell, as
 * the reference sums them) upsampled by scipy.ndimage.zoom order 1 and divided by its max; slot
 * levels + 1 = the level sum divided by its max over the batch. scratch: items * (levels + 1) + 1
 * floats. WAM_ERR_SHAPE when S is not divisible as the reference's assignment needs. */
int wam_visualize3d(int64_t items, int size, int levels, const float* cube, float* out, float* scratch,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cross-scale statistics of WAM maps and top-p mask agreement (the reference's top-level utils.py:
 * get_diagonal, get_mean_pixelwise_variance, rank_images, get_gradients_attribution_on_levels; and
 * compare_iou_models.ipynb: get_highest_percentage, iou, get_iou_between_wavelets). wam_amd/utils.py
 * drives them.
 * ---------------------------------------------------------------------------------------------- */

/* maps [images, size, size] float64, levels = J in [0, 16]. get_diagonal's blocks: detail level j
 * (j = 0 .. J - 1) is rows and columns [size / 2^(j+1), size / 2^j) (integer division), side n_j; the
 * approximation block is [0, size / 2^J). Every output may be NULL:
 *   abs_sums [images, J + 1]: sum |v| over level_0 .. level_{J-1}, then the approximation block;
 *   var_map  [images, T, T], mean_var [images] (J >= 1, T = target >= 1): each detail block is resized
 *     with scipy.ndimage.zoom(block, T / n_j, order=1)[:T, :T], var_map = np.var over the J resized
 *     levels (population variance, mean((v - mean(v))^2) with left-to-right sums), mean_var its mean.
 * out_len[J] (host): scipy's output length m_j = int(round(n_j * (T / n_j))) per level. The zoom is
 * scipy's in float64: zoom_j = (n_j - 1) / (m_j - 1), 1 when m_j == 1; output index o samples input
 * coordinate cc = zoom_j * o (one rounded multiply, no fused contraction) with i0 = floor(cc),
 * weights w0 = 1 - (cc - i0), w1 = 1 - w0, value = sum over the four taps of (v * w_row) * w_col added
 * row tap first; a tap outside [0, n_j) has weight 0 (it is read at its mirror image); a sample whose
 * coordinate rounds above n_j - 1 is 0 (mode 'constant').
 * Partial sums go to ws (wam_level_stats_ws_bytes(images, size, levels, target) bytes; target = 0
 * when neither var_map nor mean_var is asked for) and are added in a fixed order: no floating-point
 * atomics, two calls return the same bits. With var_map NULL nothing is stored for it.
 * WAM_ERR_SHAPE when some m_j < T (the reference's np.stack fails there); WAM_ERR_INVALID_ARG for a
 * detail level of side 0 with a variance output, a NULL maps, a short ws; WAM_ERR_UNSUPPORTED for
 * blocks of 2^31 elements or more (size >= 92682; size >= 46341 when levels == 0, whose one block is the map). */
int64_t wam_level_stats_ws_bytes(int64_t images, int size, int levels, int target);
int wam_level_stats(int64_t images, int size, int levels, const double* maps, int target, const int32_t* out_len,
                    double* abs_sums, double* var_map, double* mean_var, void* ws, int64_t ws_bytes,
                    void* stream);

/* maps [M, len] float64, thr [M, Q] float64 (device): pixel x of map i is selected at q when
 * maps[i, x] >= thr[i, q] (a NaN is never selected). inter / uni [Q, M (M - 1) / 2] uint64, pairs
 * (i < j) in lexicographic order: the number of pixels selected by both maps / by either map. The
 * call zeroes them itself. M in [2, 16], Q in [1, 16]: WAM_ERR_UNSUPPORTED above (the caller runs
 * pair and percentage chunks, sized by wam_mask_iou_limits: the two upper bounds of this build). */
void wam_mask_iou_limits(int* max_maps, int* max_q);
int wam_mask_iou(int M, int Q, int64_t len, const double* maps, const double* thr, uint64_t* inter, uint64_t* uni,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * 1D mel front-end (replaces lib/wam_1D.py:194-219, BaseWAM1D.compute_melspec: torchaudio
 * MelSpectrogram(sample_rate, n_fft, n_mels) with its defaults -- periodic Hann, hop n_fft / 2,
 * center + reflect padding, power 2, HTK mel without normalisation -- followed by AmplitudeToDB()
 * when to_db, and the gradient torch autograd takes through it).
 * wave [items, samples] float32 (samples > n_fft / 2); out / grad_out [items, F, n_mels] with
 * F = samples / (n_fft / 2) + 1 (the reference's [N, 1, F, n_mels] stack); n_fft a power of two
 * in [64, 2048], n_mels <= 256 (WAM_ERR_UNSUPPORTED otherwise).
 * tables (float, device): window[n_fft] | twiddle[2 n_fft] (cos, sin of -2 pi m / n_fft) |
 *   band_w[nnz] | bin_w[nnz];
 * index (int32, device): band_ptr[n_mels + 1] | band_bin[nnz] | bin_ptr[n_fft / 2 + 2] |
 *   bin_band[nnz] -- the filterbank's nonzeros by band (bins ascending) and by bin (bands
 *   ascending); wam_amd/melspec.py (MelTables) builds them from torchaudio's filterbank formula.
 * grad_wave is written (not accumulated). */
int wam_melspec(int64_t items, int64_t samples, int n_fft, int n_mels, int nnz, int to_db, const float* wave,
                const float* tables, const int32_t* index, float* out, void* stream);
int wam_melspec_adjoint(int64_t items, int64_t samples, int n_fft, int n_mels, int nnz, int to_db,
                        const float* wave, const float* grad_out, const float* tables, const int32_t* index,
                        float* grad_wave, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Explained-model input-gradient pass (lib/wam_2D.py:114-116: model forward, diag-mean loss,
 * backward). Not a ptwt replacement: fused elementwise steps of a BN-folded ReLU network, each one
 * HBM pass instead of the 2-4 torch kernels it replaces (wam_amd/model_fuse.py drives them).
 * dtype: WAM_DT_F32 or WAM_DT_BF16 (storage; arithmetic is fp32). Tensors are contiguous with n
 * elements; the channel of element i is (i / inner) % channels (inner = 1: NHWC, H*W: NCHW).
 * Bias vectors (length channels, same dtype) may be NULL (= 0). out may alias an input.
 * Special values: the forward ReLU is v < 0 ? 0 : v, so a NaN sum stays NaN (as torch.relu; max(v, 0)
 * below is written in that sense) and -0.0 may come out as either zero; the mask y > 0 ? g : 0 is 0
 * where y is -0.0, negative or NaN (torch's threshold_backward passes g at a NaN y).
 * ---------------------------------------------------------------------------------------------- */
enum wam_dtype { WAM_DT_F32 = 0, WAM_DT_BF16 = 1 };

/* y = relu ? max(y + bias[c], 0) : y + bias[c]      (in place; conv bias + ReLU) */
int wam_ew_bias_act(int dtype, int64_t n, int64_t channels, int64_t inner, void* y, const void* bias,
                    int relu, void* stream);
/* out = max((a + bias_a[c]) + (s + bias_s[c]), 0)   (residual tail of a bottleneck block) */
int wam_ew_add_bias_relu(int dtype, int64_t n, int64_t channels, int64_t inner, const void* a,
                         const void* bias_a, const void* s, const void* bias_s, void* out, void* stream);
/* out = y > 0 ? g1 (+ g2 if g2 != NULL) : 0          (ReLU backward, optionally fused fan-in) */
int wam_ew_relu_mask(int dtype, int64_t n, const void* g1, const void* g2, const void* y, void* out,
                     void* stream);
/* Packed ReLU masks. mask: uint8 [n / 8], bit i % 8 of byte i / 8 is out[i] > 0 on the stored bf16
 * value (0 for +0, -0, negatives and NaN; 1 for denormals and +inf), i the flat element index in
 * whatever layout the tensor has. The two producers store exactly what wam_ew_bias_act (relu != 0) /
 * wam_ew_add_bias_relu store and write the mask of it as well; the consumer is wam_ew_relu_mask with
 * the bit in place of y > 0, so fed a producer's mask it returns what wam_ew_relu_mask fed that
 * producer's output returns, at 1/16 of the y bytes. WAM_DT_BF16 only, n % 8 == 0, every pointer
 * (mask included) 16-byte aligned, and for the producers a channel layout with whole 16-byte vectors
 * (inner == 1 and channels % 8 == 0, or inner % 8 == 0): anything else is WAM_ERR_UNSUPPORTED with
 * nothing written (run the plain entry instead). A NULL mask is WAM_ERR_INVALID_ARG. */
int wam_ew_bias_act_bits(int dtype, int64_t n, int64_t channels, int64_t inner, void* y, const void* bias,
                         void* mask, void* stream);
int wam_ew_add_bias_relu_bits(int dtype, int64_t n, int64_t channels, int64_t inner, const void* a,
                              const void* bias_a, const void* s, const void* bias_s, void* out, void* mask,
                              void* stream);
/* out = bit ? g1 (+ g2 if g2 != NULL) : 0 */
int wam_ew_relu_mask_bits(int dtype, int64_t n, const void* g1, const void* g2, const void* mask, void* out,
                          void* stream);
/* NHWC max pooling (k x k window, stride, zero-area padding pad <= k/2, floor output size):
 * y [n, ho, wo, c], idx [n, ho, wo, c] uint8 = window position kh*k+kw | 0x80 if the max is > 0.
 * Scan order kh*k+kw over the positions inside the image, as torch: the first of equal maxima wins,
 * a NaN replaces the running maximum (the last NaN wins, bit 7 clear), a window of -inf keeps its
 * first valid position. k*k <= 127; WAM_ERR_INVALID_ARG when h + 2 pad < k or w + 2 pad < k.
 * Replaces torch max_pool2d_with_indices after the stem ReLU (torchvision ResNet maxpool);
 * WAM_ERR_UNSUPPORTED when c is not a multiple of the 16-byte vector or pointers are unaligned. */
int wam_ew_maxpool_nhwc(int dtype, int64_t n, int64_t h, int64_t w, int64_t c, int k, int stride, int pad,
                        const void* x, void* y, void* idx, void* stream);
/* wam_ew_maxpool_nhwc of relu(x + bias[c]) as wam_ew_bias_act (relu form, NHWC) stores it, taken on
 * each element as it is loaded: y and idx are what that call on x followed by the pool give, x is left
 * as it is and the biased tensor is never written. bias: c values, not NULL (WAM_ERR_INVALID_ARG),
 * 16-byte aligned (WAM_ERR_UNSUPPORTED otherwise, as for the other pointers). */
int wam_ew_bias_maxpool_nhwc(int dtype, int64_t n, int64_t h, int64_t w, int64_t c, int k, int stride, int pad,
                             const void* x, const void* bias, void* y, void* idx, void* stream);
/* gx [n, h, w, c] = sum of gy over the windows whose idx points at the pixel (fp32 sums in window
 * order); relu != 0 also drops windows whose max was not > 0 (mask of the ReLU feeding the pool). */
int wam_ew_maxpool_nhwc_backward(int dtype, int64_t n, int64_t h, int64_t w, int64_t c, int k, int stride,
                                 int pad, const void* gy, const void* idx, int relu, void* gx, void* stream);

/* Weight-stationary expanding pointwise GEMM with the neighbouring elementwise pass as its
 * epilogue (wam_amd/csrc/model_pw.hip): out[M, N] = epilogue(x[M, K] . w[N, K]^T), x / out row-major
 * (NHWC activations viewed as [N*H*W, C]), w the 1x1 convolution's weight as stored, fp32
 * accumulation, one round-to-nearest-even store. Applied to the unrounded accumulator acc:
 *   WAM_PW_TAIL: out = max((acc + bias_a[n]) + (r0[m, n] + bias_b[n]), 0)   r0 = s [M, N], r1 = NULL;
 *                either bias may be NULL (k_add_bias_relu on the accumulator; a NaN sum stays NaN)
 *   WAM_PW_MASK: out = r1[m, n] > 0 ? acc (+ r0[m, n]) : 0                  r1 = y [M, N], r0 = g2 [M, N]
 *                or NULL; biases NULL (k_relu_mask on the accumulator; 0 where y is -0.0 or NaN)
 * mode | WAM_PW_ROUNDED: acc is rounded to bf16 (nearest even) before the epilogue, i.e. the epilogue
 * sees the value a bf16 GEMM followed by wam_ew_add_bias_relu / wam_ew_relu_mask sees; results then
 * equal that pair's wherever the two fp32 accumulation orders round to the same bf16 value.
 * mode | WAM_PW_BITS: r1 is the packed ReLU mask of [M, N] (uint8 [M N / 8], the format of
 * wam_ew_add_bias_relu_bits; 16-byte aligned like the other operands). WAM_PW_TAIL writes it there,
 * from the values it stores in out (r1 must then not be NULL; it is written although the parameter
 * is declared const); WAM_PW_MASK reads it in place of y, bit set = y > 0. out is what the unflagged
 * launch gives, bit for bit; rows past M of a ragged tile write no mask byte.
 * wam_pw_supported: 1 for bf16 with (K, N) = (64, 256) or (128, 512), else 0. wam_pw_gemm returns
 * WAM_ERR_UNSUPPORTED (out untouched) for another dtype or (K, N) or when x, w, r0, r1 or out is not
 * 16-byte aligned, WAM_ERR_INVALID_ARG for M <= 0, a NULL x / w / out, an unknown mode or dtype, or
 * operands the mode does not take. out must not alias an input. wam_pw_gemm_ex caps the persistent
 * grid at max_workgroups per N split (0: the resident count), so that a test can make every
 * workgroup loop over several tiles of a small M. */
enum wam_pw_mode { WAM_PW_TAIL = 0, WAM_PW_MASK = 1, WAM_PW_ROUNDED = 16, WAM_PW_BITS = 32 };
int wam_pw_supported(int dtype, int64_t K, int64_t N);
int wam_pw_gemm(int mode, int dtype, int64_t M, int64_t K, int64_t N, const void* x, const void* w,
                const void* bias_a, const void* bias_b, const void* r0, const void* r1, void* out, void* stream);
int wam_pw_gemm_ex(int mode, int64_t M, int64_t K, int64_t N, const void* x, const void* w, const void* bias_a,
                   const void* bias_b, const void* r0, const void* r1, void* out, int max_workgroups,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAM_HIP_H */
