// Fused 3D Haar transforms for gfx950 (config c5: haar J=2 on 128^3 volumes).
//
// With the 2-tap Haar filters and dimensions divisible by 2^J no boundary extension is involved
// (p = 0, no odd-length pad), so a J-level 3D transform is local to 2^J x 2^J x 2^J blocks: one
// thread owns one block, reads it with 16-byte loads (lanes = consecutive blocks along W, so a
// wave reads whole contiguous rows), runs every level in registers and writes each band's patch
// (float2 runs at level 1 for J = 2, single values at the coarsest level). The per-axis kernels
// need 3 passes per level with intermediate volumes in HBM; this is one pass over the data.
// Arithmetic follows the per-axis kernels exactly (W then H then D; fmaf chains starting at 0),
// so results are bit-identical to the generic path.
#include "dispatch.hpp"
#include "maskexpand.hpp"
#include "rng.hpp"

namespace {

constexpr int kT3 = 256;

struct Haar3Geom {
  int J;
  int64_t D, H, W;           // input dims
  int64_t off_a;             // per-item band offsets (band-major buffer with `items` items)
  int64_t off[2][7];         // [level][key - 1]
  int64_t items;
};

// one analysis level along one axis for a pair (x0, x1) -> (lo, hi)
__device__ __forceinline__ void ana2(float x0, float x1, const float (&f)[4], float& lo, float& hi) {
  lo = fmaf(f[1], x1, fmaf(f[0], x0, 0.f));
  hi = fmaf(f[3], x1, fmaf(f[2], x0, 0.f));
}

// 2x2x2 block v[z][y][x] -> 8 subbands indexed by key = (D hi) 4 | (H hi) 2 | (W hi) 1
__device__ __forceinline__ void haar3_level(const float (&v)[2][2][2], const float (&f)[4], float (&out)[8]) {
  float w[2][2][2];  // [z][y][W part]
#pragma unroll
  for (int z = 0; z < 2; ++z)
#pragma unroll
    for (int y = 0; y < 2; ++y) ana2(v[z][y][0], v[z][y][1], f, w[z][y][0], w[z][y][1]);
  float h[2][2][2];  // [z][H part][W part]
#pragma unroll
  for (int z = 0; z < 2; ++z)
#pragma unroll
    for (int wp = 0; wp < 2; ++wp) ana2(w[z][0][wp], w[z][1][wp], f, h[z][0][wp], h[z][1][wp]);
#pragma unroll
  for (int hp = 0; hp < 2; ++hp)
#pragma unroll
    for (int wp = 0; wp < 2; ++wp) {
      float lo, hi;
      ana2(h[0][hp][wp], h[1][hp][wp], f, lo, hi);
      out[(hp << 1) | wp] = lo;
      out[4 | (hp << 1) | wp] = hi;
    }
}

// synthesis of one axis: (a, d) -> (y0, y1) = (rlo0 a + rhi0 d, rlo1 a + rhi1 d) in the
// per-axis kernel's order
__device__ __forceinline__ void syn2(float a, float d, const float (&r)[4], float& y0, float& y1) {
  y0 = fmaf(r[2], d, fmaf(r[0], a, 0.f));
  y1 = fmaf(r[3], d, fmaf(r[1], a, 0.f));
}

// 8 subbands (key order) -> 2x2x2 block; synthesis passes W, then H, then D
__device__ __forceinline__ void haar3_inv(const float (&c)[8], const float (&r)[4], float (&v)[2][2][2]) {
  float w[2][2][2];  // [D part][H part][x]
#pragma unroll
  for (int dp = 0; dp < 2; ++dp)
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) syn2(c[(dp << 2) | (hp << 1)], c[(dp << 2) | (hp << 1) | 1], r, w[dp][hp][0],
                                        w[dp][hp][1]);
  float h[2][2][2];  // [D part][y][x]
#pragma unroll
  for (int dp = 0; dp < 2; ++dp)
#pragma unroll
    for (int x = 0; x < 2; ++x) syn2(w[dp][0][x], w[dp][1][x], r, h[dp][0][x], h[dp][1][x]);
#pragma unroll
  for (int y = 0; y < 2; ++y)
#pragma unroll
    for (int x = 0; x < 2; ++x) syn2(h[0][y][x], h[1][y][x], r, v[0][y][x], v[1][y][x]);
}

// NOISE: SmoothGrad sample generation fused into the load (single-channel volumes): output item
// s * images + i is the transform of x_i + sigma_i * N(0,1) with the Philox stream of
// wam_noise_add (counter (sample_base + s, image_base + i, element / 4)); a B-wide row of a block
// is one (B = 4) or half a (B = 2) group of 4 elements, so noise costs one Philox call per row.
// Work order (NOISE): workgroup w takes sample w % S of a 256-block chunk of image w / S, so the S
// samples of a chunk are consecutive (XCD-swizzled) workgroups and read the clean chunk from one L2.
template <int J, bool NOISE>
__global__ void __launch_bounds__(kT3) k_haar3_ana(const float* __restrict__ in, float* __restrict__ coeffs,
                                                  const float* __restrict__ filt, Haar3Geom g, int64_t blocks,
                                                  WamNoise nz, int64_t S) {
  constexpr int B = 1 << J;
  const int64_t bw = g.W / B, bh = g.H / B, bd = g.D / B;
  const int64_t nb = bw * bh * bd;  // blocks per volume
  int64_t t, item, src_item, smp = 0;
  float sg = 0.f;
  if constexpr (NOISE) {
    const int64_t nc = (nb + kT3 - 1) / kT3;  // workgroup chunks per volume
    const int64_t w = wam_xcd_block(blockIdx.x, gridDim.x);
    const int64_t s = w % S, rest = w / S, i = rest / nc;
    t = (rest % nc) * kT3 + threadIdx.x;
    if (t >= nb || i >= nz.images) return;
    src_item = i;
    item = s * nz.images + i;
    smp = nz.sample_base + s;
    sg = nz.sigma[i];
  } else {
    const int64_t tt = (int64_t)blockIdx.x * kT3 + threadIdx.x;
    if (tt >= blocks) return;
    t = tt % nb;
    item = src_item = tt / nb;
  }
  const int64_t bx = t % bw, by = (t / bw) % bh, bz = t / (bw * bh);
  float f[4] = {filt[0], filt[1], filt[2], filt[3]};  // lo0 lo1 hi0 hi1
  float v[B][B][B];
  const float* src = in + src_item * g.D * g.H * g.W + (bz * B * g.H + by * B) * g.W + bx * B;
#pragma unroll
  for (int z = 0; z < B; ++z)
#pragma unroll
    for (int y = 0; y < B; ++y) {
      const float* row = src + ((int64_t)z * g.H + y) * g.W;
      if constexpr (B == 4) {
        const float4 q = *reinterpret_cast<const float4*>(row);
        v[z][y][0] = q.x;
        v[z][y][1] = q.y;
        v[z][y][2] = q.z;
        v[z][y][3] = q.w;
      } else {
        const float2 q = *reinterpret_cast<const float2*>(row);
        v[z][y][0] = q.x;
        v[z][y][1] = q.y;
      }
    }
  if constexpr (NOISE) {
    // element group of row (z, y): ((bz B + z) H + by B + y) W / 4 + bx B / 4 (W % 4 == 0, host check)
    const uint32_t W4 = (uint32_t)(g.W / 4);
    const uint32_t g0 = (uint32_t)(bz * B * g.H + by * B) * W4 + (uint32_t)(bx * B / 4);
    const uint32_t img = (uint32_t)(nz.image_base + src_item), sm = (uint32_t)smp;
#pragma unroll
    for (int r = 0; r < B * B; r += 2) {
      const int z0 = r / B, y0 = r % B, z1 = (r + 1) / B, y1 = (r + 1) % B;
      float za[4], zb[4];
      wam_normal4_x2(g0 + (uint32_t)(z0 * g.H + y0) * W4, g0 + (uint32_t)(z1 * g.H + y1) * W4, img, sm, nz.k0, nz.k1,
                     za, zb);
      const int q = (int)((bx * B) & 3);  // B = 2: the half of the group this block holds
#pragma unroll
      for (int k = 0; k < B; ++k) {
        v[z0][y0][k] = fmaf(sg, za[q + k], v[z0][y0][k]);  // noisy = fma(sigma, z, x) (wam_noise_add)
        v[z1][y1][k] = fmaf(sg, zb[q + k], v[z1][y1][k]);
      }
    }
  }
  // level 1 (finest): B/2 x B/2 x B/2 blocks of 2^3
  constexpr int B1 = B / 2;
  float ll[B1][B1][B1];
  const int64_t d1 = g.D / 2, h1 = g.H / 2, w1 = g.W / 2;
  const int64_t n1 = d1 * h1 * w1;
  float c1[B1][B1][B1][8];
#pragma unroll
  for (int z = 0; z < B1; ++z)
#pragma unroll
    for (int y = 0; y < B1; ++y)
#pragma unroll
      for (int x = 0; x < B1; ++x) {
        float blk[2][2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c) blk[a][b][c] = v[2 * z + a][2 * y + b][2 * x + c];
        haar3_level(blk, f, c1[z][y][x]);
        ll[z][y][x] = c1[z][y][x][0];
      }
  // level-1 details (level index 0 = finest)
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    float* dst = coeffs + g.items * g.off[0][k - 1] + item * n1;
#pragma unroll
    for (int z = 0; z < B1; ++z)
#pragma unroll
      for (int y = 0; y < B1; ++y) {
        const int64_t o = ((bz * B1 + z) * h1 + (by * B1 + y)) * w1 + bx * B1;
        if constexpr (B1 == 2) *reinterpret_cast<float2*>(dst + o) = make_float2(c1[z][y][0][k], c1[z][y][1][k]);
        else dst[o] = c1[z][y][0][k];
      }
  }
  if constexpr (J == 1) {
    float* dst = coeffs + g.items * g.off_a + item * n1;
    dst[(bz * h1 + by) * w1 + bx] = ll[0][0][0];
  } else {
    float c2[8];
    haar3_level(ll, f, c2);
    const int64_t d2 = d1 / 2, h2 = h1 / 2, w2 = w1 / 2;
    const int64_t n2 = d2 * h2 * w2, o = (bz * h2 + by) * w2 + bx;
    coeffs[g.items * g.off_a + item * n2 + o] = c2[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) coeffs[g.items * g.off[1][k - 1] + item * n2 + o] = c2[k];
  }
}

template <int J>
__global__ void __launch_bounds__(kT3) k_haar3_syn(const float* __restrict__ coeffs, float* __restrict__ out,
                                                  const float* __restrict__ filt, Haar3Geom g, int64_t blocks,
                                                  float s) {
  constexpr int B = 1 << J;
  constexpr int B1 = B / 2;
  const int64_t t = (int64_t)blockIdx.x * kT3 + threadIdx.x;
  if (t >= blocks) return;
  const int64_t bw = g.W / B, bh = g.H / B, bd = g.D / B;
  const int64_t bx = t % bw, by = (t / bw) % bh, bz = (t / (bw * bh)) % bd, item = t / (bw * bh * bd);
  const float r[4] = {filt[0], filt[1], filt[2], filt[3]};  // rec lo0 lo1, rec hi0 hi1
  const int64_t d1 = g.D / 2, h1 = g.H / 2, w1 = g.W / 2;
  const int64_t n1 = d1 * h1 * w1;
  float ll[B1][B1][B1];
  if constexpr (J == 1) {
    ll[0][0][0] = s * coeffs[g.items * g.off_a + item * n1 + (bz * h1 + by) * w1 + bx];
  } else {
    const int64_t h2 = h1 / 2, w2 = w1 / 2, n2 = (d1 / 2) * h2 * w2, o = (bz * h2 + by) * w2 + bx;
    float c2[8];
    c2[0] = s * coeffs[g.items * g.off_a + item * n2 + o];
#pragma unroll
    for (int k = 1; k < 8; ++k) c2[k] = s * coeffs[g.items * g.off[1][k - 1] + item * n2 + o];
    haar3_inv(c2, r, ll);  // the approximation is scaled once, on its load (as wam_waverec)
  }
  float c1[B1][B1][B1][8];
#pragma unroll
  for (int z = 0; z < B1; ++z)
#pragma unroll
    for (int y = 0; y < B1; ++y)
#pragma unroll
      for (int x = 0; x < B1; ++x) c1[z][y][x][0] = ll[z][y][x];
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const float* src = coeffs + g.items * g.off[0][k - 1] + item * n1;
#pragma unroll
    for (int z = 0; z < B1; ++z)
#pragma unroll
      for (int y = 0; y < B1; ++y) {
        const int64_t o = ((bz * B1 + z) * h1 + (by * B1 + y)) * w1 + bx * B1;
        if constexpr (B1 == 2) {
          const float2 q = *reinterpret_cast<const float2*>(src + o);
          c1[z][y][0][k] = s * q.x;
          c1[z][y][1][k] = s * q.y;
        } else {
          c1[z][y][0][k] = s * src[o];
        }
      }
  }
  float v[B][B][B];
#pragma unroll
  for (int z = 0; z < B1; ++z)
#pragma unroll
    for (int y = 0; y < B1; ++y)
#pragma unroll
      for (int x = 0; x < B1; ++x) {
        float blk[2][2][2];
        haar3_inv(c1[z][y][x], r, blk);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c) v[2 * z + a][2 * y + b][2 * x + c] = blk[a][b][c];
      }
  float* dst = out + item * g.D * g.H * g.W + (bz * B * g.H + by * B) * g.W + bx * B;
#pragma unroll
  for (int z = 0; z < B; ++z)
#pragma unroll
    for (int y = 0; y < B; ++y) {
      float* row = dst + ((int64_t)z * g.H + y) * g.W;
      if constexpr (B == 4) wam_st4(row, v[z][y][0], v[z][y][1], v[z][y][2], v[z][y][3]);
      else wam_st(reinterpret_cast<wam_f2v*>(row), wam_f2v{v[z][y][0], v[z][y][1]});
    }
}

// Ranked synthesis (wam_waverec_ranked, route 1): k_haar3_syn with the rank threshold of the
// insertion / deletion masks applied on the load. A thread reads its block's coefficients and,
// through pos, their ranks once, then walks the chunk of masks blockIdx.y names (kMaskChunk, as the
// mask expansion of maskexpand.hpp): for mask m every coefficient -- the approximation like any other
// -- is multiplied by 1.0f or 0.0f ((rank < thr(m)) != deletion, a multiply and not a select: a dropped
// NaN stays NaN), the levels are inverted in registers and the block goes to output volume
// item * (n_iter + 1) + m. The arithmetic is the expansion's multiply followed by k_haar3_syn's chains
// (whose scale is 1.0f there), so the volumes are bit-identical to that two-step route; the
// (n_iter + 1) masked coefficient sets are never stored.
template <int J>
__global__ void __launch_bounds__(kT3) k_haar3_syn_ranked(const float* __restrict__ coeffs,
                                                         const int32_t* __restrict__ rank, int64_t rank_len,
                                                         const int32_t* __restrict__ pos, float* __restrict__ out,
                                                         const float* __restrict__ filt, Haar3Geom g, int64_t blocks,
                                                         int64_t n_iter, int64_t n_comp, int deletion) {
  constexpr int B = 1 << J;
  constexpr int B1 = B / 2;
  const int64_t t = (int64_t)blockIdx.x * kT3 + threadIdx.x;
  if (t >= blocks) return;
  const int64_t bw = g.W / B, bh = g.H / B, bd = g.D / B;
  const int64_t bx = t % bw, by = (t / bw) % bh, bz = (t / (bw * bh)) % bd, item = t / (bw * bh * bd);
  const float r[4] = {filt[0], filt[1], filt[2], filt[3]};  // rec lo0 lo1, rec hi0 hi1
  const int32_t* rk = rank + item * rank_len;
  const int64_t d1 = g.D / 2, h1 = g.H / 2, w1 = g.W / 2;
  const int64_t n1 = d1 * h1 * w1;
  // coarsest level: J = 1 the approximation alone (slot 0 of the level-1 block), J = 2 eight bands
  float c2[8];
  int32_t r2[8];
  float c1[B1][B1][B1][8];
  int32_t r1[B1][B1][B1][8];
  if constexpr (J == 1) {
    const int64_t o = (bz * h1 + by) * w1 + bx;
    c1[0][0][0][0] = coeffs[g.items * g.off_a + item * n1 + o];
    r1[0][0][0][0] = slot_rank(rk, pos[g.off_a + o], rank_len);
  } else {
    const int64_t h2 = h1 / 2, w2 = w1 / 2, n2 = (d1 / 2) * h2 * w2, o = (bz * h2 + by) * w2 + bx;
    c2[0] = coeffs[g.items * g.off_a + item * n2 + o];
    r2[0] = slot_rank(rk, pos[g.off_a + o], rank_len);
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      c2[k] = coeffs[g.items * g.off[1][k - 1] + item * n2 + o];
      r2[k] = slot_rank(rk, pos[g.off[1][k - 1] + o], rank_len);
    }
  }
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const float* src = coeffs + g.items * g.off[0][k - 1] + item * n1;
    const int32_t* ps = pos + g.off[0][k - 1];
#pragma unroll
    for (int z = 0; z < B1; ++z)
#pragma unroll
      for (int y = 0; y < B1; ++y) {
        const int64_t o = ((bz * B1 + z) * h1 + (by * B1 + y)) * w1 + bx * B1;
        if constexpr (B1 == 2) {
          const float2 q = *reinterpret_cast<const float2*>(src + o);
          const int2 pq = *reinterpret_cast<const int2*>(ps + o);
          c1[z][y][0][k] = q.x;
          c1[z][y][1][k] = q.y;
          r1[z][y][0][k] = slot_rank(rk, pq.x, rank_len);
          r1[z][y][1][k] = slot_rank(rk, pq.y, rank_len);
        } else {
          c1[z][y][0][k] = src[o];
          r1[z][y][0][k] = slot_rank(rk, ps[o], rank_len);
        }
      }
  }
  const int64_t M = n_iter + 1, vol = g.D * g.H * g.W;
  const int64_t m0 = (int64_t)blockIdx.y * kMaskChunk;
  const int64_t m1 = m0 + kMaskChunk < M ? m0 + kMaskChunk : M;
  const bool del = deletion != 0;
  float* dst0 = out + item * M * vol + (bz * B * g.H + by * B) * g.W + bx * B;
#pragma unroll 1
  for (int64_t m = m0; m < m1; ++m) {
    const int32_t thr = (int32_t)mask_thr(m, n_iter, n_comp, rank_len);  // rank_len <= INT32_MAX (host check)
    auto keep = [&](int32_t rv) { return ((rv < thr) != del) ? 1.f : 0.f; };
    float ll[B1][B1][B1];
    if constexpr (J == 1) {
      ll[0][0][0] = c1[0][0][0][0] * keep(r1[0][0][0][0]);
    } else {
      float cm[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) cm[k] = c2[k] * keep(r2[k]);
      haar3_inv(cm, r, ll);
    }
    float* dst = dst0 + m * vol;
#pragma unroll
    for (int z = 0; z < B1; ++z)
#pragma unroll
      for (int y = 0; y < B1; ++y) {
        float v[2][2][B];  // rows (2z + a, 2y + b) of the block
#pragma unroll
        for (int x = 0; x < B1; ++x) {
          float cm[8], blk[2][2][2];
          cm[0] = ll[z][y][x];
#pragma unroll
          for (int k = 1; k < 8; ++k) cm[k] = c1[z][y][x][k] * keep(r1[z][y][x][k]);
          haar3_inv(cm, r, blk);
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) v[a][b][2 * x] = blk[a][b][0], v[a][b][2 * x + 1] = blk[a][b][1];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            float* row = dst + ((int64_t)(2 * z + a) * g.H + (2 * y + b)) * g.W;
            if constexpr (B == 4) wam_st4(row, v[a][b][0], v[a][b][1], v[a][b][2], v[a][b][3]);
            else wam_st(reinterpret_cast<wam_f2v*>(row), wam_f2v{v[a][b][0], v[a][b][1]});
          }
      }
  }
}

// Cell-mask synthesis (wam_waverec_cells, route 1): k_haar3_syn_ranked with float masks looked up through
// a coefficient -> grid-cell table instead of a rank threshold. The grid is (blocks of one volume, chunks
// of masks, sets), so a workgroup serves one set and `chunk` of its mask rows (the launcher's choice, at
// most kMaskChunk). A thread reads its block's coefficients and slots once -- a slot outside [0, grid_len)
// becomes column grid_len, which reads as 1.0f -- then for every mask of the chunk multiplies (c * f, one
// fp32 multiply: NaN * 0 stays NaN), inverts the levels in registers and stores the block. The arithmetic
// is the expansion's multiply followed by k_haar3_syn's chains with scale 1: bit-identical to route 0.
// STAGE = false, the default, gathers f from the mask's row in global memory: the rows are small (512
// floats at the default grid) and stay in the caches. STAGE = true (-DWAM_CELLS_LDS=1, kernels.hpp) stages
// the chunk's rows in LDS first, grid_len + 1 floats per row whose last is 1.0f, so that the lookup is one
// LDS read without a compare. The direct form measured 3 to 4 % faster at 128^3, the same at 16^3 J = 1
// and 6 % slower at 16^3 J = 2 (profiles/eval3d_cells_kbench.txt), and it has no LDS bound on grid_len.
template <int J, bool STAGE>
__global__ void __launch_bounds__(kT3) k_haar3_syn_cells(const float* __restrict__ coeffs,
                                                        const int32_t* __restrict__ slot, int64_t n_masks,
                                                        int grid_len, const float* __restrict__ grid,
                                                        float* __restrict__ out, const float* __restrict__ filt,
                                                        Haar3Geom g, int64_t nb, int chunk) {
  constexpr int B = 1 << J;
  constexpr int B1 = B / 2;
  extern __shared__ float cell_rows[];  // [masks of the chunk][grid_len + 1]
  const int64_t item = blockIdx.z;
  const int T = blockDim.x;  // kT3, or the waves that hold a small volume's blocks
  const int64_t m0 = (int64_t)blockIdx.y * chunk;
  const int64_t m1 = m0 + chunk < n_masks ? m0 + chunk : n_masks;
  const int stride = grid_len + 1;
  const float* grow0 = grid + (item * n_masks + m0) * grid_len;
  if constexpr (STAGE) {
    const int nrow = (int)(m1 - m0);
    for (int r = 0; r < nrow; ++r) {
      for (int c = threadIdx.x; c < grid_len; c += T) cell_rows[r * stride + c] = grow0[(int64_t)r * grid_len + c];
      if (threadIdx.x == 0) cell_rows[r * stride + grid_len] = 1.0f;
    }
    __syncthreads();
  }
  const int64_t t = (int64_t)blockIdx.x * T + threadIdx.x;
  if (t >= nb) return;
  const int64_t bw = g.W / B, bh = g.H / B;
  const int64_t bx = t % bw, by = (t / bw) % bh, bz = t / (bw * bh);
  const float r[4] = {filt[0], filt[1], filt[2], filt[3]};  // rec lo0 lo1, rec hi0 hi1
  // a slot outside [0, grid_len) becomes column grid_len; grid_len <= kCellsMaxGrid, so a column fits 16
  // bits and two share a register (64 slots at J = 2: 32 VGPRs less, which keeps two waves per SIMD)
  auto col = [&](int32_t s) { return (uint32_t)((uint32_t)s < (uint32_t)grid_len ? s : grid_len); };
  auto put = [](uint32_t(&w)[4], int k, uint32_t c) { w[k >> 1] |= c << ((k & 1) * 16); };
  auto get = [](const uint32_t(&w)[4], int k) { return (int)((w[k >> 1] >> ((k & 1) * 16)) & 0xffffu); };
  const int64_t d1 = g.D / 2, h1 = g.H / 2, w1 = g.W / 2;
  const int64_t n1 = d1 * h1 * w1;
  float c2[8];
  uint32_t s2[4] = {0, 0, 0, 0};
  float c1[B1][B1][B1][8];
  uint32_t s1[B1][B1][B1][4];
#pragma unroll
  for (int z = 0; z < B1; ++z)
#pragma unroll
    for (int y = 0; y < B1; ++y)
#pragma unroll
      for (int x = 0; x < B1; ++x)
#pragma unroll
        for (int q = 0; q < 4; ++q) s1[z][y][x][q] = 0;
  if constexpr (J == 1) {
    const int64_t o = (bz * h1 + by) * w1 + bx;
    c1[0][0][0][0] = coeffs[g.items * g.off_a + item * n1 + o];
    put(s1[0][0][0], 0, col(slot[g.off_a + o]));
  } else {
    const int64_t h2 = h1 / 2, w2 = w1 / 2, n2 = (d1 / 2) * h2 * w2, o = (bz * h2 + by) * w2 + bx;
    c2[0] = coeffs[g.items * g.off_a + item * n2 + o];
    put(s2, 0, col(slot[g.off_a + o]));
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      c2[k] = coeffs[g.items * g.off[1][k - 1] + item * n2 + o];
      put(s2, k, col(slot[g.off[1][k - 1] + o]));
    }
  }
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const float* src = coeffs + g.items * g.off[0][k - 1] + item * n1;
    const int32_t* ss = slot + g.off[0][k - 1];
#pragma unroll
    for (int z = 0; z < B1; ++z)
#pragma unroll
      for (int y = 0; y < B1; ++y) {
        const int64_t o = ((bz * B1 + z) * h1 + (by * B1 + y)) * w1 + bx * B1;
        if constexpr (B1 == 2) {
          const float2 q = *reinterpret_cast<const float2*>(src + o);
          const int2 sq = *reinterpret_cast<const int2*>(ss + o);
          c1[z][y][0][k] = q.x;
          c1[z][y][1][k] = q.y;
          put(s1[z][y][0], k, col(sq.x));
          put(s1[z][y][1], k, col(sq.y));
        } else {
          c1[z][y][0][k] = src[o];
          put(s1[z][y][0], k, col(ss[o]));
        }
      }
  }
  const int64_t vol = g.D * g.H * g.W;
  float* dst0 = out + item * n_masks * vol + (bz * B * g.H + by * B) * g.W + bx * B;
#pragma unroll 1
  for (int64_t m = m0; m < m1; ++m) {
    // the packed columns are unpacked per mask: without this the unpacking is hoisted out of the loop and
    // the 64 columns of J = 2 take a register each again (262 VGPRs, one wave per SIMD)
    if constexpr (J == 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(s2[q]));
    }
#pragma unroll
    for (int z = 0; z < B1; ++z)
#pragma unroll
      for (int y = 0; y < B1; ++y)
#pragma unroll
        for (int x = 0; x < B1; ++x)
#pragma unroll
          for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(s1[z][y][x][q]));
    const float* lrow = cell_rows + (int)(m - m0) * stride;
    const float* grow = grow0 + (m - m0) * grid_len;
    auto f = [&](int s) {
      if constexpr (STAGE) return lrow[s];
      else return s < grid_len ? grow[s] : 1.0f;
    };
    float ll[B1][B1][B1];
    if constexpr (J == 1) {
      ll[0][0][0] = c1[0][0][0][0] * f(get(s1[0][0][0], 0));
    } else {
      float cm[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) cm[k] = c2[k] * f(get(s2, k));
      haar3_inv(cm, r, ll);
    }
    float* dst = dst0 + m * vol;
#pragma unroll
    for (int z = 0; z < B1; ++z)
#pragma unroll
      for (int y = 0; y < B1; ++y) {
        float v[2][2][B];  // rows (2z + a, 2y + b) of the block
#pragma unroll
        for (int x = 0; x < B1; ++x) {
          float cm[8], blk[2][2][2];
          cm[0] = ll[z][y][x];
#pragma unroll
          for (int k = 1; k < 8; ++k) cm[k] = c1[z][y][x][k] * f(get(s1[z][y][x], k));
          haar3_inv(cm, r, blk);
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) v[a][b][2 * x] = blk[a][b][0], v[a][b][2 * x + 1] = blk[a][b][1];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            float* row = dst + ((int64_t)(2 * z + a) * g.H + (2 * y + b)) * g.W;
            if constexpr (B == 4) wam_st4(row, v[a][b][0], v[a][b][1], v[a][b][2], v[a][b][3]);
            else wam_st(reinterpret_cast<wam_f2v*>(row), wam_f2v{v[a][b][0], v[a][b][1]});
          }
      }
  }
}

Haar3Geom make_geom3(const wam_plan* p, int64_t items) {
  Haar3Geom g{};
  g.J = p->levels;
  g.D = p->lin[0][0];
  g.H = p->lin[0][1];
  g.W = p->lin[0][2];
  g.off_a = p->band_off[0];
  for (int l = 0; l < p->levels; ++l)
    for (int k = 0; k < 7; ++k) g.off[l][k] = p->band_off[wam_band_of(p, l, k)];
  g.items = items;
  return g;
}

}  // namespace

bool dwt3_haar_supported(const wam_plan* p) {
  if (p->ndim != 3 || p->L != 2 || p->levels < 1 || p->levels > 2) return false;
  const int B = 1 << p->levels;
  for (int a = 0; a < 3; ++a)
    if (p->lin[0][a] % B) return false;
  return true;  // no padding for even sizes: every boundary mode gives the same coefficients
}

int launch_dwt3_haar_analysis(const wam_plan* p, int64_t batch, const float* in, float* coeffs, bool adjoint,
                              hipStream_t st) {
  if (!dwt3_haar_supported(p) || ((uintptr_t)in & 15)) return WAM_ERR_UNSUPPORTED;
  const Haar3Geom g = make_geom3(p, batch);
  const int B = 1 << p->levels;
  const int64_t blocks = batch * (g.D / B) * (g.H / B) * (g.W / B);
  const int64_t grid = (blocks + kT3 - 1) / kT3;
  if (grid > 0x7fffffff) return WAM_ERR_UNSUPPORTED;
  const float* filt = p->d_filt + (adjoint ? WAM_F_ADJ_LO : WAM_F_ANA_LO) * p->L;  // lo0 lo1 hi0 hi1
  WamTimer tm(st, "k_haar3_ana", 4.0 * (double)batch * ((double)g.D * g.H * g.W + (double)p->band_off[p->nbands]));
  if (p->levels == 1)
    hipLaunchKernelGGL((k_haar3_ana<1, false>), dim3((unsigned)grid), dim3(kT3), 0, st, in, coeffs, filt, g, blocks,
                       kNoNoise, (int64_t)1);
  else
    hipLaunchKernelGGL((k_haar3_ana<2, false>), dim3((unsigned)grid), dim3(kT3), 0, st, in, coeffs, filt, g, blocks,
                       kNoNoise, (int64_t)1);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int launch_dwt3_haar_analysis_noisy(const wam_plan* p, int64_t batch, const float* in, float* coeffs,
                                    const WamNoise* nz, int64_t n_samples, hipStream_t st) {
  if (!dwt3_haar_supported(p) || ((uintptr_t)in & 15) || !nz) return WAM_ERR_UNSUPPORTED;
  if (nz->channels != 1 || batch != n_samples * nz->images) return WAM_ERR_UNSUPPORTED;
  const Haar3Geom g = make_geom3(p, batch);
  if (g.W % 4 || g.D * g.H * g.W >= (int64_t(1) << 34)) return WAM_ERR_UNSUPPORTED;  // 32-bit element groups
  const int B = 1 << p->levels;
  const int64_t nb = (g.D / B) * (g.H / B) * (g.W / B);
  const int64_t grid = n_samples * nz->images * ((nb + kT3 - 1) / kT3);
  if (grid > 0x7fffffff) return WAM_ERR_UNSUPPORTED;
  const float* filt = p->d_filt + WAM_F_ANA_LO * p->L;
  const double vol = (double)g.D * g.H * g.W;
  // algorithmic bytes: the clean volumes once, every sample's coefficients
  WamTimer tm(st, "k_haar3_ana<noise>", 4.0 * ((double)nz->images * vol + (double)batch * p->band_off[p->nbands]));
  if (p->levels == 1)
    hipLaunchKernelGGL((k_haar3_ana<1, true>), dim3((unsigned)grid), dim3(kT3), 0, st, in, coeffs, filt, g, batch * nb,
                       *nz, n_samples);
  else
    hipLaunchKernelGGL((k_haar3_ana<2, true>), dim3((unsigned)grid), dim3(kT3), 0, st, in, coeffs, filt, g, batch * nb,
                       *nz, n_samples);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

int launch_dwt3_haar_synthesis(const wam_plan* p, int64_t batch, const float* coeffs, const float* alpha, int n_alpha,
                               float* out, hipStream_t st) {
  if (!dwt3_haar_supported(p) || ((uintptr_t)out & 15)) return WAM_ERR_UNSUPPORTED;
  const Haar3Geom g = make_geom3(p, batch);
  const int B = 1 << p->levels;
  const int64_t blocks = batch * (g.D / B) * (g.H / B) * (g.W / B);
  const int64_t grid = (blocks + kT3 - 1) / kT3;
  if (grid > 0x7fffffff) return WAM_ERR_UNSUPPORTED;
  const float* filt = p->d_filt + WAM_F_SYN_LO * p->L;  // rec lo0 lo1 hi0 hi1
  const int64_t vol = g.D * g.H * g.W;
  for (int ai = 0; ai < n_alpha; ++ai) {
    const float s = alpha ? alpha[ai] : 1.0f;
    float* o = out + (int64_t)ai * batch * vol;
    WamTimer tm(st, "k_haar3_syn", 4.0 * (double)batch * ((double)vol + (double)p->band_off[p->nbands]));
    if (p->levels == 1)
      hipLaunchKernelGGL(k_haar3_syn<1>, dim3((unsigned)grid), dim3(kT3), 0, st, coeffs, o, filt, g, blocks, s);
    else
      hipLaunchKernelGGL(k_haar3_syn<2>, dim3((unsigned)grid), dim3(kT3), 0, st, coeffs, o, filt, g, blocks, s);
    WAM_LAUNCH_CHECK();
  }
  return WAM_OK;
}

// The fused route of wam_waverec_ranked. Declines (WAM_ERR_UNSUPPORTED) what the kernel's vector
// accesses cannot take: out not 16-byte, coeffs or pos not 8-byte aligned.
int launch_dwt3_haar_synthesis_ranked(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* rank,
                                      int64_t rank_len, const int32_t* pos, int64_t n_iter, int64_t n_comp,
                                      int deletion, float* out, hipStream_t st) {
  if (!dwt3_haar_supported(p) || !aligned16(out) || ((uintptr_t)coeffs & 7) || ((uintptr_t)pos & 7))
    return WAM_ERR_UNSUPPORTED;
  const Haar3Geom g = make_geom3(p, sets);
  const int B = 1 << p->levels;
  const int64_t blocks = sets * (g.D / B) * (g.H / B) * (g.W / B);
  const int64_t grid = (blocks + kT3 - 1) / kT3, M = n_iter + 1, chunks = (M + kMaskChunk - 1) / kMaskChunk;
  if (grid > 0x7fffffff) return WAM_ERR_UNSUPPORTED;
  if (chunks > 65535) return WAM_ERR_INVALID_ARG;
  const float* filt = p->d_filt + WAM_F_SYN_LO * p->L;  // rec lo0 lo1 hi0 hi1
  const double K = (double)p->band_off[p->nbands];
  WamTimer tm(st, "k_haar3_syn_ranked",
              4.0 * (sets * K + (double)sets * rank_len + K + (double)sets * M * g.D * g.H * g.W));
  const dim3 gd((unsigned)grid, (unsigned)chunks);
  if (p->levels == 1)
    hipLaunchKernelGGL(k_haar3_syn_ranked<1>, gd, dim3(kT3), 0, st, coeffs, rank, rank_len, pos, out, filt, g, blocks,
                       n_iter, n_comp, deletion);
  else
    hipLaunchKernelGGL(k_haar3_syn_ranked<2>, gd, dim3(kT3), 0, st, coeffs, rank, rank_len, pos, out, filt, g, blocks,
                       n_iter, n_comp, deletion);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}

// The fused route of wam_waverec_cells. Declines (WAM_ERR_UNSUPPORTED) what the kernel cannot take: out
// not 16-byte, coeffs or slot not 8-byte aligned, a grid_len above kCellsMaxGrid (its 16-bit columns),
// more sets than gridDim.z holds.
int launch_dwt3_haar_synthesis_cells(const wam_plan* p, int64_t sets, const float* coeffs, const int32_t* slot,
                                     int64_t n_masks, int64_t grid_len, const float* grid, float* out,
                                     hipStream_t st) {
  if (!dwt3_haar_supported(p) || !aligned16(out) || ((uintptr_t)coeffs & 7) || ((uintptr_t)slot & 7) ||
      grid_len > kCellsMaxGrid || sets > 65535)
    return WAM_ERR_UNSUPPORTED;
  const Haar3Geom g = make_geom3(p, sets);
  const int B = 1 << p->levels;
  const int64_t nb = (g.D / B) * (g.H / B) * (g.W / B);
  // A volume of fewer than kT3 blocks takes the waves that hold them. A thread keeps its coefficients for
  // a chunk of kMaskChunk masks; where that leaves the chip short of work (16^3 at J = 2: 64 blocks per
  // volume, one wave per set and chunk) the chunk is halved until the grid holds two waves per SIMD, the
  // residency of the J = 2 kernel, or a mask per workgroup: the coefficients are re-read from L2.
  const int threads = nb < kT3 ? (int)((nb + 63) / 64 * 64) : kT3;
  const int64_t gx = (nb + threads - 1) / threads;
  if (gx > 0x7fffffff) return WAM_ERR_UNSUPPORTED;
  if ((n_masks + kMaskChunk - 1) / kMaskChunk > 65535) return WAM_ERR_INVALID_ARG;
  int cus = 0;
  WAM_HIP_CHECK(wam_device_cus(&cus));
  int chunk = kMaskChunk;
  while (chunk > 1 && gx * (threads / 64) * ((n_masks + chunk - 1) / chunk) * sets < 8 * (int64_t)cus &&
         (n_masks + chunk / 2 - 1) / (chunk / 2) <= 65535)
    chunk /= 2;
  const int64_t chunks = (n_masks + chunk - 1) / chunk;
  const float* filt = p->d_filt + WAM_F_SYN_LO * p->L;  // rec lo0 lo1 hi0 hi1
  const double K = (double)p->band_off[p->nbands];
  constexpr bool kStage = WAM_CELLS_LDS != 0;
  const int64_t rows = n_masks < chunk ? n_masks : chunk;
  const size_t lds = kStage ? (size_t)(rows * (grid_len + 1)) * sizeof(float) : 0;
  WamTimer tm(st, "k_haar3_syn_cells",
              4.0 * (sets * K + K + (double)sets * n_masks * grid_len + (double)sets * n_masks * g.D * g.H * g.W));
  const dim3 gd((unsigned)gx, (unsigned)chunks, (unsigned)sets);
  if (p->levels == 1)
    hipLaunchKernelGGL((k_haar3_syn_cells<1, kStage>), gd, dim3(threads), lds, st, coeffs, slot, n_masks,
                       (int)grid_len, grid, out, filt, g, nb, chunk);
  else
    hipLaunchKernelGGL((k_haar3_syn_cells<2, kStage>), gd, dim3(threads), lds, st, coeffs, slot, n_masks,
                       (int)grid_len, grid, out, filt, g, nb, chunk);
  WAM_LAUNCH_CHECK();
  return WAM_OK;
}
