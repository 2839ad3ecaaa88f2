// Adjoint of the boundary-extended, stride-2 analysis: the backward pass of wam_wavedec with
// respect to the analysed signal (what autograd computes through ptwt.wavedec*).
//
// Per axis of one level (n input samples, L taps, p = L - 2, padl = p, padr = p + n % 2,
// m = (n + padl + padr - L) / 2 + 1 outputs, T = n + padl + padr = 2m - 2 + L extended samples):
//   y[t]  = sum_j f_lo[t - 2j] glo[j] + f_hi[t - 2j] ghi[j]        0 <= t < T, 0 <= t - 2j < L
//   gx[i] = sum of y[t] over the t in [0, T) with wam_ext_index(t - padl, n, mode) == i
// with f_lo / f_hi the arrays the analysis correlates with (WAM_F_ANA_LO / HI). y is a
// synthesis-shaped pass (a transposed convolution with the analysis filters); the sum folds its
// padded tails t < padl and t >= padl + n back onto the signal. Every output gathers its own terms in
// a fixed order (no atomics): two runs give the same bits.
//
// Two routes:
//   axis    k_analysis_adjoint_axis, one launch per axis and filter pair as the other per-axis
//           kernels (dwt_axis.hip): any ndim, any even L, every mode, any n >= 1 (an index then has
//           as many preimages as the tails hold). Serves every plan.
//   fold2d  one 2D level as interior + border: the interior term y[i + padl] is the streaming level
//           synthesis (k_dwt2_syn, dwt2_fused.hip) run with the analysis filters onto the level's
//           input dims; k_dwt2_adjoint_border then adds, to the outputs whose row or column has a
//           preimage in a tail (strips about p wide along the four edges), the tail terms gathered
//           straight from the four band planes. Needs n > p on both axes (the strips then hold every
//           folded index); skipped in zero mode, where nothing folds.
#include "dispatch.hpp"
#include "kernels.hpp"

namespace {

// y[t] of one line: lo / hi point at element 0 of the line, consecutive elements `inner` apart
__device__ __forceinline__ float adj_y(const float* __restrict__ plo, const float* __restrict__ phi, int64_t inner,
                                       int m, int t, const float* __restrict__ flo,
                                       const float* __restrict__ fhi, int L) {
  int jmax = t >> 1;
  if (jmax > m - 1) jmax = m - 1;
  int jmin = (t - L + 2) >> 1;  // ceil((t - L + 1) / 2)
  if (jmin < 0) jmin = 0;
  float y = 0.f;
  for (int j = jmax; j >= jmin; --j) {
    const int k = t - 2 * j;
    y = fmaf(flo[k], plo[(int64_t)j * inner], y);
    y = fmaf(fhi[k], phi[(int64_t)j * inner], y);
  }
  return y;
}

__global__ void __launch_bounds__(256) k_analysis_adjoint_axis(const float* __restrict__ lo,
                                                               const float* __restrict__ hi,
                                                               float* __restrict__ gx, int64_t outer, int m, int n,
                                                               int64_t inner, int padl, int mode,
                                                               const float* __restrict__ flo,
                                                               const float* __restrict__ fhi, int L) {
  const int64_t total = outer * (int64_t)n * inner;
  const int T = 2 * m - 2 + L;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e % inner;
    const int64_t q = e / inner;
    const int i = (int)(q % n);
    const int64_t o = q / n;
    const float* plo = lo + o * (int64_t)m * inner + r;
    const float* phi = hi + o * (int64_t)m * inner + r;
    float acc = adj_y(plo, phi, inner, m, i + padl, flo, fhi, L);
    // the tails: for n > padl every folded index lies within padl + 2 of an end
    if (mode != WAM_MODE_ZERO && (n <= padl || i <= padl || i >= n - padl - 2)) {
      for (int t = 0; t < padl; ++t)
        if (wam_ext_index(t - padl, n, mode) == i) acc += adj_y(plo, phi, inner, m, t, flo, fhi, L);
      for (int t = padl + n; t < T; ++t)
        if (wam_ext_index(t - padl, n, mode) == i) acc += adj_y(plo, phi, inner, m, t, flo, fhi, L);
    }
    gx[(o * n + i) * inner + r] = acc;
  }
}

// The border strips of an axis of n samples: indices [0, wl) and [n - wr, n), all of [0, n) when
// the two meet (nb == n). strip_index: the k-th of them; strip_slot: its inverse, -1 outside.
__device__ __forceinline__ int strip_index(int k, int n, int nb, int wl, int wr) {
  return (nb == n || k < wl) ? k : n - wr + (k - wl);
}
__device__ __forceinline__ int strip_slot(int i, int n, int nb, int wl, int wr) {
  if (nb == n || i < wl) return i;
  return i >= n - wr ? i - (n - wr) + wl : -1;
}

// The tails of an axis that fold onto index i, found by one wave: lane b tests tail position
// t = (b < p ? b : n + b); bit b of the (wave-uniform) result is set when it maps onto i. The tails
// hold 2p + n % 2 <= 37 positions.
__device__ __forceinline__ uint64_t tail_mask(int i, int n, int p, int T, int mode, int lane) {
  const int t = lane < p ? lane : n + lane;
  const bool hit = t < T && wam_ext_index(t - p, n, mode) == i;
  return (uint64_t)__ballot(hit);
}
__device__ __forceinline__ int tail_pos(int bit, int n, int p) { return bit < p ? bit : n + bit; }

constexpr int kMaxStrip = 2 * 18 + 3;  // wl + wr = 2p + 3 at L = 20
constexpr int kBorderCW = 256;         // output columns of a row-pass workgroup
constexpr int kBorderRG = 8;           // strip rows of a row-pass workgroup
constexpr int kBorderRH = 32;          // output rows of a column-pass workgroup

// The folded tail terms of one level, separably. With Y[tr, tc] the 2D transposed convolution at an
// extended position, output (r, c) lacks, after the interior pass,
//   sum over tail rows tr -> r of Y[tr, c + p]                     (row term)
//   sum over tail columns tc -> c of Y[r + p, tc]                  (column term)
//   sum over both of Y[tr, tc]                                     (corner term)
// Two launches, both adding into the interior pass's output. The row pass (a workgroup per
// kBorderRG strip rows and kBorderCW columns) filters the bands down the tail rows into LDS (per
// strip row two lines of coefficients, the tail rows of r summed), then along the columns: the row
// term of every column, and the corner term of the strip columns from the same lines (gathered
// directly where a tail column's coefficients lie outside the workgroup's lines: periodic planes
// wider than kBorderCW). The column pass (a workgroup per kBorderRH rows, all strip columns) does the
// same transposed for the column term. The filters sit in LDS: a lane picks its taps by the parity
// of its extended position.
template <int L>
__global__ void __launch_bounds__(256) k_dwt2_adjoint_border(const float* __restrict__ A, const float* __restrict__ H,
                                                             const float* __restrict__ V, const float* __restrict__ D,
                                                             int mh, int mw, float* __restrict__ out, int nh, int nw,
                                                             int mode, const float* __restrict__ filt, int nbr,
                                                             int nbc, int wl, int wr, int nchc, int ngr, int nchr,
                                                             bool rows) {
  constexpr int p = L - 2, H2 = L / 2;
  constexpr int NJC = kBorderCW / 2 + H2;      // coefficient columns under kBorderCW outputs
  constexpr int NJR = kBorderRH / 2 + H2 + 1;  // coefficient rows under kBorderRH outputs
  constexpr int WS = kMaxStrip * NJR > kBorderRG * NJC ? kMaxStrip * NJR : kBorderRG * NJC;
  __shared__ uint64_t cmk[kMaxStrip], rmk[kBorderRG];
  __shared__ float ws[2][WS];
  __shared__ float sf[2 * L];  // lo taps, then hi taps
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int Th = 2 * mh - 2 + L, Tw = 2 * mw - 2 + L;
  const int64_t b = blockIdx.x;
  const int64_t plane = rows ? b / ((int64_t)ngr * nchc) : b / nchr;
  const int k0 = rows ? (int)(b % ngr) * kBorderRG : 0;  // first strip row of a row-pass workgroup
  const int nrow = rows ? min(kBorderRG, nbr - k0) : 0;
  if (tid < 2 * L) sf[tid] = filt[tid];
  for (int k = wv; k < nbc; k += 4) {
    const uint64_t mk = tail_mask(strip_index(k, nw, nbc, wl, wr), nw, p, Tw, mode, lane);
    if (lane == 0) cmk[k] = mk;
  }
  for (int i = wv; i < nrow; i += 4) {
    const uint64_t mk = tail_mask(strip_index(k0 + i, nh, nbr, wl, wr), nh, p, Th, mode, lane);
    if (lane == 0) rmk[i] = mk;
  }
  __syncthreads();
  const float* flo = sf;
  const float* fhi = sf + L;
  const int64_t in_plane = (int64_t)mh * mw, out_plane = (int64_t)nh * nw;
  const float* pa = A + plane * in_plane;
  const float* ph = H + plane * in_plane;
  const float* pv = V + plane * in_plane;
  const float* pd = D + plane * in_plane;
  float* po = out + plane * out_plane;

  if (rows) {
    const int c0 = (int)((b / ngr) % nchc) * kBorderCW;
    const int jlo = ((c0 + p) >> 1) - (H2 - 1);  // = c0 / 2
    // the bands filtered down the tail rows of each strip row: (A, H) -> its lo line, (V, D) -> its hi line
    for (int it = tid; it < nrow * NJC; it += 256) {
      const int i = it / NJC, jc = jlo + it % NJC;
      float sl = 0.f, sh = 0.f;
      if (jc >= 0 && jc < mw) {
        for (uint64_t rm = rmk[i]; rm; rm &= rm - 1) {
          const int tr = tail_pos(__ffsll((unsigned long long)rm) - 1, nh, p);
          const int par = tr & 1, jr0 = tr >> 1;
          for (int ir = 0; ir < H2; ++ir) {
            const int jr = jr0 - ir;
            if (jr < 0 || jr >= mh) continue;
            const float lr = flo[par + 2 * ir], hr = fhi[par + 2 * ir];
            const int64_t o = (int64_t)jr * mw + jc;
            sl = fmaf(lr, pa[o], sl);
            sl = fmaf(hr, ph[o], sl);
            sh = fmaf(lr, pv[o], sh);
            sh = fmaf(hr, pd[o], sh);
          }
        }
      }
      ws[0][it] = sl;
      ws[1][it] = sh;
    }
    __syncthreads();
    for (int it = tid; it < nrow * kBorderCW; it += 256) {
      const int i = it / kBorderCW, t = it % kBorderCW;
      const int c = c0 + t;
      const uint64_t rmask = rmk[i];
      if (c >= nw || !rmask) continue;  // no tail row folds onto this strip row (the strips are a superset)
      const int r = strip_index(k0 + i, nh, nbr, wl, wr);
      const float* llo = ws[0] + i * NJC;
      const float* lhi = ws[1] + i * NJC;
      // the line entry of coefficient column jc is jc - jlo; c0 + p is even, so output c0 + t sits over
      // entries (t >> 1) + H2 - 1 downwards
      auto along = [&](int tc, int first) {
        const int par = tc & 1;
        float y = 0.f;
        for (int ic = 0; ic < H2; ++ic) {
          const int e = first - ic;
          // tail columns only: a coefficient column left of the plane (jlo = c0 / 2 >= 0) or, right of
          // it, past the lines (which hold 0 from column mw on)
          if (e < 0 || e >= NJC) continue;
          y = fmaf(flo[par + 2 * ic], llo[e], y);
          y = fmaf(fhi[par + 2 * ic], lhi[e], y);
        }
        return y;
      };
      float acc = along(c + p, (t >> 1) + H2 - 1);
      const int kc = strip_slot(c, nw, nbc, wl, wr);
      if (kc >= 0) {  // the corner term
        for (uint64_t cm = cmk[kc]; cm; cm &= cm - 1) {
          const int tc = tail_pos(__ffsll((unsigned long long)cm) - 1, nw, p);
          // coefficient columns max(tc / 2 - H2 + 1, 0) .. min(tc / 2, mw - 1) of the lines
          const int hi = min(tc >> 1, mw - 1) - jlo, lo = max((tc >> 1) - (H2 - 1), 0) - jlo;
          if (lo >= 0 && hi < NJC) {  // every coefficient column inside the plane is in the lines
            acc += along(tc, (tc >> 1) - jlo);
            continue;
          }
          const int qar = tc & 1, jc0 = tc >> 1;  // gathered directly
          for (uint64_t rm = rmask; rm; rm &= rm - 1) {
            const int tr = tail_pos(__ffsll((unsigned long long)rm) - 1, nh, p);
            const int par = tr & 1, jr0 = tr >> 1;
            for (int ir = 0; ir < H2; ++ir) {
              const int jr = jr0 - ir;
              if (jr < 0 || jr >= mh) continue;
              float sl = 0.f, sh = 0.f;
              for (int ic = 0; ic < H2; ++ic) {
                const int jc = jc0 - ic;
                if (jc < 0 || jc >= mw) continue;
                const float lc = flo[qar + 2 * ic], hc = fhi[qar + 2 * ic];
                const int64_t o = (int64_t)jr * mw + jc;
                sl = fmaf(lc, pa[o], sl);
                sl = fmaf(hc, pv[o], sl);
                sh = fmaf(lc, ph[o], sh);
                sh = fmaf(hc, pd[o], sh);
              }
              acc = fmaf(flo[par + 2 * ir], sl, acc);
              acc = fmaf(fhi[par + 2 * ir], sh, acc);
            }
          }
        }
      }
      po[(int64_t)r * nw + c] += acc;
    }
    return;
  }

  // the column term of every row: kBorderRH rows from r0 (even, as p is)
  const int r0 = (int)(b % nchr) * kBorderRH;
  const int jlo = ((r0 + p) >> 1) - (H2 - 1);  // = r0 / 2
  // the bands filtered along the tail columns of each strip column: (A, V) -> its lo line, (H, D) -> its hi line
  for (int it = tid; it < NJR * nbc; it += 256) {
    const int k = it % nbc, t = it / nbc;
    const int jr = jlo + t;
    float sl = 0.f, sh = 0.f;
    if (jr >= 0 && jr < mh) {
      for (uint64_t cm = cmk[k]; cm; cm &= cm - 1) {
        const int tc = tail_pos(__ffsll((unsigned long long)cm) - 1, nw, p);
        const int par = tc & 1, jc0 = tc >> 1;
        for (int ic = 0; ic < H2; ++ic) {
          const int jc = jc0 - ic;
          if (jc < 0 || jc >= mw) continue;
          const float lc = flo[par + 2 * ic], hc = fhi[par + 2 * ic];
          const int64_t o = (int64_t)jr * mw + jc;
          sl = fmaf(lc, pa[o], sl);
          sl = fmaf(hc, pv[o], sl);
          sh = fmaf(lc, ph[o], sh);
          sh = fmaf(hc, pd[o], sh);
        }
      }
    }
    ws[0][k * NJR + t] = sl;
    ws[1][k * NJR + t] = sh;
  }
  __syncthreads();
  const int rend = min(nh, r0 + kBorderRH);
  for (int it = tid; it < kBorderRH * nbc; it += 256) {
    const int k = it % nbc, r = r0 + it / nbc;
    if (r >= rend || !cmk[k]) continue;
    const int tr = r + p;
    const int par = tr & 1;
    const int base = k * NJR + (tr >> 1) - jlo;  // entries base - (H2 - 1) .. base lie in line k
    float acc = 0.f;
    for (int ir = 0; ir < H2; ++ir) {
      acc = fmaf(flo[par + 2 * ir], ws[0][base - ir], acc);
      acc = fmaf(fhi[par + 2 * ir], ws[1][base - ir], acc);
    }
    po[(int64_t)r * nw + strip_index(k, nw, nbc, wl, wr)] += acc;
  }
}

}  // namespace

int launch_analysis_adjoint_axis(const float* lo, const float* hi, float* gx, int64_t outer, int m, int n,
                                 int64_t inner, int padl, int mode, const float* flo, const float* fhi, int L,
                                 hipStream_t st) {
  int64_t work = outer * (int64_t)n * inner;
  if (work == 0) return WAM_OK;
  WamTimer tm(st, "k_analysis_adjoint_axis", 4.0 * (double)outer * inner * (2.0 * m + n));
  hipLaunchKernelGGL(k_analysis_adjoint_axis, dim3(wam_grid(work, 256)), dim3(256), 0, st, lo, hi, gx, outer, m, n,
                     inner, padl, mode, flo, fhi, L);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

bool dwt2_adjoint_fold_supported(const wam_plan* p, int level) {
  return dwt2_fused_supported(p) && p->lin[level][0] > p->pad && p->lin[level][1] > p->pad;
}

int launch_dwt2_adjoint_fold(const wam_plan* p, int64_t batch, int level, const float* a, const float* const* sub,
                             float* out, hipStream_t st) {
  const int nh = (int)p->lin[level][0], nw = (int)p->lin[level][1];
  const int mh = (int)p->lout[level][0], mw = (int)p->lout[level][1];
  SynBatch sb{};
  sb.na = 1;
  sb.a[0] = a;
  sb.out[0] = out;
  sb.sa[0] = 1.0f;
  sb.sd[0] = 1.0f;
  int rc = launch_dwt2_synthesis_fused_to(p, batch, level, sb, sub, WAM_F_ANA_LO, nh, nw, st);
  if (rc || p->mode == WAM_MODE_ZERO) return rc;
  // strips wide enough for every mode: a tail of p (+ 1 at the far end of an odd axis) positions
  // lands within p + 1 of the near end or p + 2 of the far end (the kernel tests each index exactly)
  const int wl = p->pad + 1, wr = p->pad + 2;
  const int nbr = wl + wr >= nh ? nh : wl + wr;
  const int nbc = wl + wr >= nw ? nw : wl + wr;
  const int nchc = (nw + kBorderCW - 1) / kBorderCW;
  const int nchr = (nh + kBorderRH - 1) / kBorderRH;
  const int ngr = (nbr + kBorderRG - 1) / kBorderRG;
  const int64_t row_groups = batch * ngr * nchc, col_groups = batch * nchr;
  if (row_groups > 0x7fffffff || col_groups > 0x7fffffff) return WAM_ERR_UNSUPPORTED;
  const float* filt = p->d_filt + WAM_F_ANA_LO * p->L;
  for (int pass = 0; pass < 2; ++pass) {
    const bool rows = pass == 0;
    // bytes: the pass's strips read and written once, and half as many coefficients under them (a
    // quarter in each of the four bands, twice)
    const double strip = rows ? (double)nbr * nw : (double)nh * nbc;
    WamTimer tm(st, "k_dwt2_adjoint_border", 4.0 * 2.5 * (double)batch * strip);
    const dim3 grid((unsigned)(rows ? row_groups : col_groups));
    if (int rc = wam_dispatch_len(WamLensEven20{}, p->L, [&](auto l) -> int {
          hipLaunchKernelGGL(k_dwt2_adjoint_border<decltype(l)::value>, grid, dim3(256), 0, st, a, sub[0], sub[1],
                             sub[2], mh, mw, out, nh, nw, p->mode, filt, nbr, nbc, wl, wr, nchc, ngr, nchr, rows);
          return WAM_OK;
        }))
      return rc;
    WAM_LAUNCH_CHECK();
  }
  return WAM_OK;
}
