"""What the evaluators (evaluation.py, baselines.py, baselines_audio.py, analysis.py) share on the host:
rankings, the audio evaluators' ranking-to-masked-rows step and source spectrogram, the softmax / AUC of
stacked logits, cached device tables (array layout, superpixel cell map), the
show() normalisation, the default transform's resize and the ImageNet constants."""
import math
import random

import numpy as np
import torch
from scipy.ndimage import zoom

from ._lib import c_f32, check, lib, ptr, stream_of
from .melspec import kernel_supported, mel_forward, melspec_db

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_TABLES = {}


def norm_consts(C):
    """(mean, std) of the first C ImageNet channels as the C arrays the kernels take."""
    return (c_f32 * C)(*IMAGENET_MEAN[:C]), (c_f32 * C)(*IMAGENET_STD[:C])


# ------------------------------------------------------------------------------ rankings and curves
def check_tie_order(tie_order):
    if tie_order not in ("stable", "numpy"):
        raise ValueError("tie_order must be 'stable' or 'numpy'")
    return tie_order


def descending_ranks(values, dev, tie_order):
    """values [sets, P] (host): int32 [sets, P] on `dev`, rank[s, p] = position of p in set s's descending
    order of the values as given (signed: generate_masks has no abs). Ties: 'numpy' ranks on the host with
    np.argsort like the reference (not stable, differs across numpy builds), 'stable' on the device."""
    values = np.ascontiguousarray(values)
    if tie_order == "numpy":
        order = torch.as_tensor(np.stack([np.argsort(v, axis=None)[::-1] for v in values])).to(dev)
    else:
        order = torch.argsort(torch.as_tensor(values).to(dev), dim=1, stable=True).flip(1)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(order.shape[1], device=dev).expand_as(order))
    return rank.to(torch.int32).contiguous()


def rank_mask_rows(explanation, source, n_iter, deletion, dev, tie_order):
    """auc_from_melspec of both audio evaluators (src/evaluators.py:145-176, 394-425) for one clip
    ([T, n_mels] explanation and dB mel spectrogram) or a batch of clips ([sets, T, n_mels]): the ranking
    of the signed explanation (generate_masks has no abs) --wam_rank_mask_rows--> the n_iter + 1 masked
    spectrograms of every clip, [sets * (n_iter + 1), 1, T, n_mels] float32 on the device."""
    expl = np.asarray(explanation)
    expl = expl.reshape((-1,) + expl.shape[-2:])
    src = torch.as_tensor(source).detach().to(dev, torch.float32).reshape(expl.shape).contiguous()
    sets, n = expl.shape[0], expl.shape[1] * expl.shape[2]
    rank = descending_ranks(expl.reshape(sets, n), dev, tie_order)
    out = torch.empty((sets * (n_iter + 1), 1) + expl.shape[1:], dtype=torch.float32, device=dev)
    check(lib.wam_rank_mask_rows(sets, n, ptr(src), ptr(rank), n_iter, int(n / n_iter), int(bool(deletion)), ptr(out),
                                 stream_of(dev)))
    return out


def db_melspec(wave, n_fft, sample_rate, n_mels):
    """The dB mel spectrogram the audio evaluators mask, wave [N, L] float32 (device) -> [N, 1, T, n_mels]:
    k_mel_fwd where it applies, else the torch path."""
    if kernel_supported(n_fft, n_mels):
        return mel_forward(wave, n_fft, sample_rate, n_mels).unsqueeze(1)
    return melspec_db(wave, n_fft, sample_rate, n_mels)


def softmax(preds):
    return np.exp(preds) / np.sum(np.exp(preds), axis=1, keepdims=True)


def compute_auc(probs):
    """src/evaluation_helpers.py:437-453."""
    return sum(probs) / (np.max(probs) * len(probs))


def class_probs(model, inputs, label):
    """Model forward (no grad) -> the reference's host softmax -> probabilities of `label`."""
    with torch.no_grad():
        return softmax(model(inputs).float().cpu().numpy())[:, label]


def class_curves(preds, M, labels):
    """preds [len(labels) * M, classes] logits of stacked sets -> per set the probabilities [M] of its label
    (arrays of preds' dtype; the AUC's dtype path and the return type are the caller's)."""
    return [softmax(preds[k * M:(k + 1) * M])[:, label] for k, label in enumerate(labels)]


def generate_subsets(grid_size, subset_size, sample_size):
    """src/evaluation_helpers.py:580-594 (Python's global random, as the reference)."""
    return [[(i // grid_size, i % grid_size) for i in random.sample(range(grid_size * grid_size), subset_size)]
            for _ in range(sample_size)]


# ------------------------------------------------------------------------------ host geometry, device tables
def coeff_array_layout(plan):
    """pywt.coeffs_to_array positions (row-major flat index) of a plan's band-major item and the
    array shape: A at [0:ah, 0:aw]; per level (coarsest first) 'da' (= cH, ptwt 'horizontal')
    rows [ah:ah+dh] x cols [0:dw], 'ad' (cV) rows [0:dh] x cols [aw:aw+dw], 'dd' at
    [ah:, aw:]; then (ah, aw) += (dh, dw)."""
    J = plan.levels
    ah, aw = plan.band_shapes[0]
    H = ah + sum(plan.band_shapes[1 + 3 * l][0] for l in range(J))
    W = aw + sum(plan.band_shapes[1 + 3 * l][1] for l in range(J))
    parts = [(np.arange(ah)[:, None] * W + np.arange(aw)[None, :]).reshape(-1)]
    for l in range(J):
        dh, dw = plan.band_shapes[1 + 3 * l + 2]
        for b, (r0, c0) in enumerate(((ah, 0), (0, aw), (ah, aw))):
            h, w = plan.band_shapes[1 + 3 * l + b]
            parts.append(((r0 + np.arange(h))[:, None] * W + (c0 + np.arange(w))[None, :]).reshape(-1))
        ah, aw = ah + dh, aw + dw
    return np.concatenate(parts), (H, W)


def zoom_cell_map(grid, hw):
    """scipy.ndimage.zoom(masks, (1, H / grid, W / grid), order=0) as a per-pixel grid-cell
    index map (zoom of the cell-index grid: nearest neighbour copies values exactly)."""
    idx = np.arange(grid * grid, dtype=np.float64).reshape(1, grid, grid)
    return zoom(idx, (1, hw[0] / grid, hw[1] / grid), order=0)[0].astype(np.int64)


def zoom_cell_map3(grid, S):
    """scipy.ndimage.zoom(masks, (1, S / grid, S / grid, S / grid), order=0) of [n, grid, grid, grid] masks
    as a per-voxel grid-cell index map, int64 [S, S, S] (cells in C order): the zoom of the cell-index
    volume, nearest neighbour copies values exactly. ValueError unless the result is (S, S, S) and every
    cell holds a voxel."""
    grid, S = int(grid), int(S)
    if grid < 1 or S < 1:
        raise ValueError("zoom_cell_map3: grid_size %d and volume size %d must be positive" % (grid, S))
    idx = np.arange(grid ** 3, dtype=np.float64).reshape(grid, grid, grid)
    cell = np.rint(zoom(idx, (S / grid,) * 3, order=0)).astype(np.int64)
    if cell.shape != (S, S, S) or np.unique(cell).size != grid ** 3:
        raise ValueError("a %d^3 superpixel grid does not cover a %d^3 volume with every cell non-empty "
                         "(zoomed to %s, %d of %d cells used)" % (grid, S, cell.shape, np.unique(cell).size, grid ** 3))
    return cell


def gaussian_weights(sigma, truncate=4.0):
    """scipy's _gaussian_kernel1d(sigma, 0, int(truncate * sigma + 0.5)): w[j] for |offset| j."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[r:], r


def device_table(key, make):
    """make() -- a host-built table moved to the device -- once per key (the key names the device)."""
    if key not in _TABLES:
        _TABLES[key] = make()
    return _TABLES[key]


def array_layout(plan, dev):
    """coeff_array_layout of a plan as (int32 positions on `dev`, array shape), cached."""
    def make():
        pos, shape = coeff_array_layout(plan)
        return torch.as_tensor(pos.astype(np.int32)).to(dev), shape
    return device_table((plan, dev), make)


def cell_map(grid_size, hw, dev):
    """zoom_cell_map as flat int32 [H * W] on `dev`, cached."""
    return device_table((grid_size, tuple(hw), dev), lambda: torch.as_tensor(
        zoom_cell_map(grid_size, hw).astype(np.int32)).to(dev).reshape(-1))


def cell_map3(grid_size, S, dev):
    """zoom_cell_map3 as flat int32 [S^3] on `dev`, cached."""
    return device_table(("cells3", int(grid_size), int(S), dev), lambda: torch.as_tensor(
        zoom_cell_map3(grid_size, S).astype(np.int32)).to(dev).reshape(-1))


def masked_sums(values, subsets, cell):
    """wam_masked_sums (sum_importance, src/evaluation_helpers.py:361-393): values float64 [H * W] on the
    device (or [S^3] of a volume), subsets [n, grid, grid] (or [n, grid, grid, grid]) float32 (host), cell
    from cell_map (cell_map3) -> per subset the float64 sum of
    the values under its upsampled mask, numpy [n]."""
    dev = values.device
    subd = torch.as_tensor(subsets).to(dev)
    out = torch.empty(subd.shape[0], dtype=torch.float64, device=dev)
    check(lib.wam_masked_sums(subd.shape[0], values.numel(), ptr(values), subd[0].numel(), ptr(subd), ptr(cell),
                              ptr(out), stream_of(dev)))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------ images and the default transform
def show_images(x, dev):
    """show(x[i]) (src/helpers.py:421-448) on the device: a list of [3, H, W] float32 tensors, min-max
    normalised per image when outside [0, 1] (numpy: img -= min; img /= max)."""
    xd = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
    out = []
    for i in range(xd.shape[0]):
        img = xd[i]
        mn, mx = img.min(), img.max()
        if bool(mx > 1) or bool(mn < 0):
            img = img - mn
            img = img / img.max()
        out.append(img)
    return out


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow's resample tables for BILINEAR along one axis (libImaging/Resample.c precompute_coeffs
    with box (0, in_size), then normalize_coeffs_8bpc): (ksize, bounds [out, 2] = (first source
    index, count), 22-bit fixed-point weights [out, ksize] int64, C truncation of w * 2^22 +- 0.5)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                      # the triangle filter's support is 1
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize))
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww = 0.0
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - t if t < 1.0 else 0.0
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            kk[xx, :xmax] /= ww
        bounds[xx] = (xmin, xmax)
    fixed = np.trunc(np.where(kk < 0, -0.5 + kk * (1 << 22), 0.5 + kk * (1 << 22))).astype(np.int64)
    return ksize, bounds, fixed


def resize_default(dev, rec, M, C, rh, rw, mean, std, size=(224, 224), rule=0):
    """The default transform on a reconstruction of another size: uint8 quantisation (rule 0: min-max,
    rule 1: the analyzer's), Pillow's BILINEAR resample to 224 x 224 (what torchvision's Resize does to
    the reference's PIL image) and ToTensor + Normalize, on the device
    (wam_quantize_resize_normalize_ex). Returns (model inputs, the quantised bytes [M, C, rh * rw])."""
    oh, ow = size
    th = tv = None
    if ow != rw:
        th = pil_bilinear_coeffs(rw, ow)
    if oh != rh:
        tv = pil_bilinear_coeffs(rh, oh)
    y0, tmp_h = 0, rh
    if th is not None and tv is not None:  # the horizontal pass covers the rows the vertical one reads
        b = tv[1]
        y0, tmp_h = int(b[0, 0]), int(b[-1, 0] + b[-1, 1] - b[0, 0])
        tv = (tv[0], b - np.array([y0, 0], dtype=b.dtype), tv[2])
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    bh = kh = bv = kv = None
    if th is not None:
        bh, kh = dv(th[1]), dv(th[2])
    if tv is not None:
        bv, kv = dv(tv[1]), dv(tv[2])
    scratch = torch.empty(M * C * (rh * rw + (tmp_h * ow if th is not None else 0)) + 16, dtype=torch.uint8,
                          device=dev)
    out = torch.empty((M, C, oh, ow), dtype=torch.float32, device=dev)
    p_ = lambda t: None if t is None else ptr(t)  # noqa: E731
    check(lib.wam_quantize_resize_normalize_ex(M, C, rh, rw, ptr(rec), rule, oh, ow, th[0] if th else 0, p_(bh),
                                               p_(kh), tv[0] if tv else 0, p_(bv), p_(kv), y0, tmp_h, mean, std,
                                               ptr(scratch), ptr(out), stream_of(dev)))
    return out, scratch[:M * C * rh * rw].view(M, C, rh * rw)
