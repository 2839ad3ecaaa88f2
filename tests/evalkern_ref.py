"""Plain-numpy references of the oldest evaluator's entries of include/wam_hip.h (the kernels of
wam_amd/csrc/evaluate.hip): wam_gaussian_filter2d, wam_rank_masks, wam_coeff_masks, wam_upsample_masks,
wam_masked_sums and the Pillow resample behind wam_quantize_resize_normalize_ex. Written from the
header's contract sentences; no torch and no project code. Arithmetic is float64, or float32 where the
kernel's contract is float32; numpy rounds every operation to nearest even and never fuses a multiply
with an add. tests/test_evalkern_ref.py pins each reference to scipy, Pillow and the float64 oracle.

The second half builds the inputs of the GPU cases (tests/test_gpu_evalkern.py), so that the host tests
can state the premise of a case -- a transposed or mis-strided variant of the reference differs from
the reference -- on the very input the kernel is given. The keyword arguments marked `variant` switch
one indexing rule of a reference the wrong way; they exist for those premises only.

Layouts (as the header): coefficients band-major (band b of `items` planes: [items, n_b] at
items * off[b]); masks [n_masks, mask_len]; pos [K] per packed coefficient of one plane.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53        # float64 unit roundoff
SENTINEL = -7777.0      # what the GPU tests fill guards and untouched outputs with (exact in fp32 and fp64)
WORST = {}              # largest error / bound ratio seen by assert_sum_bound, per entry


# ------------------------------------------------------------------------------ comparators
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_bits(got, ref, what, nan_as_value=False):
    """got equals ref bit for bit (-0.0 is not 0.0). nan_as_value: NaN exactly where ref has NaN, with
    any sign or payload (the sign of inf * 0 differs between hosts and the GPU), bits elsewhere."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    same = bits(got) == bits(ref)
    if nan_as_value:
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN at other elements than the reference" % what
        same = same | np.isnan(ref)
    assert same.all(), "%s: %d of %d elements differ from the reference, first at %s" % (
        what, (~same).sum(), same.size, np.argwhere(~same)[0])


def assert_sum_bound(got, ref, S, n, what):
    """|got - fsum| <= (n + 1) * 2^-53 * S per mask: any summation order of n rounded products, S the sum
    of their magnitudes. Prints and records the largest error / bound ratio."""
    got, ref, S = (np.asarray(v, dtype=F64) for v in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (what, got.shape, ref.shape, S.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all() and (S > 0).all(), what
    ratio = np.abs(got - ref) / ((n + 1) * U64 * S)
    worst = float(ratio.max()) if ratio.size else 0.0
    key = what.split()[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("[evalkern] %s: max error / bound = %.3g over %d masks" % (what, worst, ratio.size))
    assert worst <= 1.0, "%s: error / bound = %.3g" % (what, worst)
    return worst


# ------------------------------------------------------------------------------ gaussian
def gaussian_weights(sigma, truncate=4.0):
    """scipy's _gaussian_kernel1d(sigma, 0, r), r = int(truncate * sigma + 0.5): (w[j] for offset +-j, r)."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:]), r


def symmetric_index(i, n):
    """half-sample symmetric extension (d c b a | a b c d | d c b a) of any index: per = 2n, i mod per,
    mirrored -- it reflects any number of times."""
    r = np.mod(i, 2 * n)
    return np.where(r >= n, 2 * n - 1 - r, r)


def gauss_pass(x, w, r, axis):
    """one 1-D pass: acc = x0 * w0; for j = r..1: acc = acc + (x[-j] + x[+j]) * w[j], every operation
    rounded."""
    x = np.asarray(x, dtype=F64)
    n = x.shape[axis]
    idx = np.arange(n)
    acc = x * F64(w[0])
    for j in range(r, 0, -1):
        lo = np.take(x, symmetric_index(idx - j, n), axis=axis)
        hi = np.take(x, symmetric_index(idx + j, n), axis=axis)
        acc = acc + (lo + hi) * F64(w[j])
    return acc


def gaussian_ref(x, w, r, axes=(0, 1)):
    """wam_gaussian_filter2d: x [items, h, w] float64, axis 0 of every item, then axis 1. `axes` (variant):
    the axis of each of the two passes."""
    x = np.asarray(x, dtype=F64)
    assert x.ndim == 3 and len(w) >= r + 1
    return gauss_pass(gauss_pass(x, w, r, 1 + axes[0]), w, r, 1 + axes[1])


# ------------------------------------------------------------------------------ ranking masks
def rank_masks_ref(rank, n_iter, n_comp, length, deletion):
    """wam_rank_masks: masks [n_iter + 1, len] float32, mask m = 1 where rank < thr(m): thr(0) = 0,
    thr(m) = min(m * n_comp, len) for m < n_iter, thr(n_iter) = len; deletion: the complement."""
    rank = np.asarray(rank, dtype=np.int64).reshape(-1)
    assert rank.size == length
    out = np.empty((n_iter + 1, length), dtype=F32)
    for m in range(n_iter + 1):
        thr = 0 if m == 0 else (length if m >= n_iter else min(m * n_comp, length))
        keep = rank < thr
        out[m] = np.where(keep != bool(deletion), F32(1), F32(0))
    return out


# ------------------------------------------------------------------------------ coefficient masks
def coeff_masks_ref(band_off, items, coeffs, pos, n_masks, mask_len, masks, mask_stride=None, out_band_items=None):
    """wam_coeff_masks: coeffs flat band-major over `items` planes, pos [K] int32 (< mask_len), masks
    [n_masks, mask_len] float32 -> flat band-major float32 over n_masks * items planes, plane (m, i) =
    m * items + i, every value the single float32 product coeffs * masks[m, pos]. Variants: mask_stride
    (row stride of masks, default mask_len), out_band_items (planes per band on the output side, default
    n_masks * items)."""
    nb = len(band_off) - 1
    K = band_off[nb]
    coeffs = np.asarray(coeffs, dtype=F32).reshape(-1)
    mflat = np.asarray(masks, dtype=F32).reshape(-1)
    pos = np.asarray(pos, dtype=np.int64).reshape(-1)
    assert coeffs.size == items * K and pos.size == K and mflat.size == n_masks * mask_len
    assert pos.size == 0 or (pos.min() >= 0 and pos.max() < mask_len)
    stride = mask_len if mask_stride is None else mask_stride
    planes = n_masks * items
    obi = planes if out_band_items is None else out_band_items
    out = np.full(planes * K, F32(SENTINEL), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(nb):
            bn = band_off[b + 1] - band_off[b]
            src = coeffs[items * band_off[b]:items * band_off[b + 1]].reshape(items, bn)
            p = pos[band_off[b]:band_off[b + 1]]
            for m in range(n_masks):
                mv = mflat[m * stride + p]
                o = obi * band_off[b] + m * items * bn
                out[o:o + items * bn] = (src * mv[None, :]).reshape(-1)
    assert out.dtype == F32
    return out


# ------------------------------------------------------------------------------ superpixel masks
def upsample_ref(masks, hw):
    """wam_upsample_masks: scipy.ndimage.zoom(masks, (1, H / grid, W / grid), order=0) of the float masks
    themselves [n, grid, grid] -> [n, H, W] (not through a cell map)."""
    from scipy.ndimage import zoom
    masks = np.asarray(masks, dtype=F32)
    grid = masks.shape[1]
    out = zoom(masks, (1, hw[0] / grid, hw[1] / grid), order=0)
    assert out.shape == (masks.shape[0],) + tuple(hw) and out.dtype == F32
    return out


def masked_sums_ref(wam, grid, cell):
    """wam_masked_sums: (sum_m, S_m) with sum_m = math.fsum over p of wam[p] * float64(grid[m, cell[p]]) --
    the correctly rounded sum of the rounded float64 products -- and S_m = fsum of their magnitudes."""
    wam = np.asarray(wam, dtype=F64).reshape(-1)
    cell = np.asarray(cell, dtype=np.int64).reshape(-1)
    grid = np.asarray(grid, dtype=F32)
    g = grid.reshape(grid.shape[0], -1)
    assert cell.size == wam.size and cell.min() >= 0 and cell.max() < g.shape[1]
    sums, mags = np.empty(g.shape[0]), np.empty(g.shape[0])
    for m in range(g.shape[0]):
        terms = wam * g[m, cell].astype(F64)
        sums[m] = math.fsum(terms)
        mags[m] = math.fsum(np.abs(terms))
    return sums, mags


# ------------------------------------------------------------------------------ Pillow resample
def pil_resize_ref(u8, size, mean, std):
    """The default transform on bytes: u8 [images, C, h, w] -> float32 [images, C, oh, ow]; each image as
    HWC through the real PIL.Image.resize((ow, oh), BILINEAR), then (u / 255 - mean) / std as float32
    divisions and a subtraction, in the kernel's order."""
    from PIL import Image
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 4 and u8.shape[1] == 3
    oh, ow = size
    m = np.asarray(mean, dtype=F32)[:, None, None]
    sd = np.asarray(std, dtype=F32)[:, None, None]
    out = np.empty((u8.shape[0], u8.shape[1], oh, ow), dtype=F32)
    for i, img in enumerate(u8):
        hwc = np.ascontiguousarray(np.moveaxis(img, 0, 2))
        res = np.asarray(Image.fromarray(hwc).resize((ow, oh), Image.BILINEAR))
        assert res.shape == (oh, ow, 3) and res.dtype == np.uint8
        q = np.moveaxis(res, 2, 0).astype(F32)
        out[i] = (q / F32(255) - m) / sd
    assert out.dtype == F32
    return out


# ------------------------------------------------------------------------------ the GPU cases' inputs
# wam_gaussian_filter2d, (items, h, w, sigma); sigma 8 -> radius 32, more than twice either extent of 8 x 12;
# sigma 16 -> radius 64, the accepted maximum
GAUSS_CASES = [(3, 37, 52, 2), (2, 52, 37, 2), (1, 5, 37, 2), (1, 37, 5, 2), (2, 1, 9, 2), (2, 9, 1, 2), (1, 3, 3, 2),
               (1, 8, 12, 8), (1, 20, 24, 16)]


def gauss_input(items, h, w, seed=0):
    """items of different data: signed noise on a per-item ramp, a different scale per item."""
    rng = np.random.RandomState(1000 * h + w + seed)
    per_item = np.arange(items)[:, None, None]
    x = rng.standard_normal((items, h, w)) + np.linspace(-1, 2, h * w).reshape(1, h, w) * (1 + per_item)
    return np.ascontiguousarray(x * 1.5 ** per_item)


# wam_rank_masks, (len, n_iter, n_comp)
RANK_CASES = [(1924, 8, 240), (1924, 7, 274), (1924, 1, 1924), (5, 8, 0), (100, 4, 60)]


def rank_rows(length):
    """(a permutation, a row with repeated rank values) int32."""
    rng = np.random.RandomState(length)
    perm = rng.permutation(length).astype(np.int32)
    return perm, (perm // 7 * 7).astype(np.int32)


# wam_coeff_masks, name -> (wavelet, filter length, (H, W), J), all in symmetric mode
COEFF_PLANS = {"db4_37x52_J2": ("db4", 8, (37, 52), 2), "db2_40x56_J2": ("db2", 4, (40, 56), 2),
               "haar_24x40_J3": ("haar", 2, (24, 40), 3), "sym4_33x20_J1": ("sym4", 8, (33, 20), 1)}


def band_layout(hw, L, J):
    """band shapes [A, (H, V, D) coarsest first ...] and per-plane offsets of a 2-D wavedec in symmetric
    mode: pywt's dwt_coeff_len, (n + L - 1) // 2 per axis and level."""
    h, w = hw
    levels = []
    for _ in range(J):
        h, w = (h + L - 1) // 2, (w + L - 1) // 2
        levels.append((h, w))
    shapes = [levels[-1]] + [s for s in reversed(levels) for _ in range(3)]
    off = np.concatenate([[0], np.cumsum([a * b for a, b in shapes])])
    return shapes, [int(v) for v in off]


def extra_slot_pos(pos, cells, seed=0):
    """the mosaic layout's form: about 5 % of the coefficients point at the extra slot `cells` (mask_len =
    cells + 1)."""
    rng = np.random.RandomState(seed + len(pos))
    out = np.array(pos, dtype=np.int32)
    out[rng.uniform(size=out.size) < 0.05] = cells
    return out


def coeff_input(band_off, items, n_masks, pos, mask_len, seed=0):
    """(coeffs flat band-major float32 with one +inf and one NaN, masks [n_masks, mask_len] float32 uniform
    in [-2, 2] with some exact 0.0, -0.0 and 1.0). The +inf coefficient meets a 0.0 of mask 0 (NaN in the
    reference) and, with more masks, a non-zero value of mask 1 (+-inf)."""
    K = band_off[-1]
    rng = np.random.RandomState(seed + 7 * items + n_masks + mask_len)
    coeffs = (rng.standard_normal(items * K) * 3).astype(F32)
    masks = rng.uniform(-2, 2, (n_masks, mask_len)).astype(F32)
    pick = rng.uniform(size=masks.shape)
    masks[pick < 0.05] = F32(0.0)
    masks[(pick >= 0.05) & (pick < 0.10)] = F32(-0.0)
    masks[(pick >= 0.10) & (pick < 0.15)] = F32(1.0)
    b = len(band_off) - 2                     # the last band: its first plane's element 3 and last plane's last
    bn = band_off[b + 1] - band_off[b]
    coeffs[items * band_off[b] + 3] = np.inf
    coeffs[items * band_off[b] + items * bn - 1] = np.nan
    masks[0, pos[band_off[b] + 3]] = F32(0.0)
    if n_masks > 1:
        masks[1, pos[band_off[b] + 3]] = F32(-1.5)
    return coeffs, masks


# wam_upsample_masks and the geometry of wam_masked_sums, (grid, (H, W))
ZOOM_CASES = [(5, (15, 17)), (7, (37, 52)), (28, (244, 244)), (8, (61, 100)), (3, (2, 11))]


def grid_masks(n_masks, grid, seed=0):
    """random signed float masks [n_masks, grid, grid], nothing binary about them."""
    rng = np.random.RandomState(seed + 31 * n_masks + grid)
    return (rng.standard_normal((n_masks, grid, grid)) * 1.7).astype(F32)


# wam_masked_sums, (len, (H, W), grid): below, at and just past the 256-thread workgroup, two ragged maps
SUMS_CASES = [(255, (15, 17), 5), (256, (16, 16), 5), (257, (1, 257), 5), (1924, (37, 52), 7), (50176, (224, 224), 28)]


def sums_input(length, n_masks, grid, seed=0):
    """(wam [2, len] float64, grid masks [n_masks, grid, grid] float32). Map 0 is positive; map 1 has mixed
    signs and zero mean, and mask 0 is constant 1.25, so that its sum over map 1 is near zero next to S_0
    (the bound is about S_m, not about the result)."""
    rng = np.random.RandomState(seed + length + n_masks)
    a = rng.standard_normal(length) * 10.0
    wam = np.stack([rng.uniform(0.1, 3.0, length), a - a.mean()])
    g = grid_masks(n_masks, grid, seed + 5)
    g[0] = F32(1.25)
    return wam, g


# the Pillow resample, (rh, rw) -> (oh, ow)
RESIZE_CASES = [((100, 224), (224, 224)),   # vertical-only, up-scale
                ((300, 224), (224, 224)),   # vertical-only, down-scale
                ((512, 512), (224, 224)),   # ksize 7 on both axes
                ((50, 120), (16, 20)),      # x3.1 and x6: ksize 9 and 13
                ((97, 61), (224, 224))]     # mixed up-scale on both axes


def resize_input(rh, rw, rule):
    """3 reconstructions of 3 channels [3, 3, rh * rw] float32; image 1 is constant."""
    rng = np.random.RandomState(rh + 3 * rw + rule)
    rec = rng.uniform(-0.3, 1.1, (3, 3, rh * rw)).astype(F32)
    rec[1] = F32(0.25)
    return rec
