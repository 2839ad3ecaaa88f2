"""Plain-numpy float64 restatement of Eval2DWAM(mask_layout="mosaic") (TEST INFRASTRUCTURE).

The reference evaluates in pywt's coeffs_to_array layout only, so this restates the definition the
class documents from parts the reference does have: the slice assignments of visualize_grad_wam
(lib/wam_2D.py:233, 238-261) to find the cell of every coefficient, generate_masks' threshold rule on the
WAM's cells (thr(m) = m * int(Hc * Wc / n_iter), the last mask forced full), float64 oracle.dwt.wavedec2
/ waverec2 in mode 'symmetric', and the quantisation, transform, softmax, AUC, subsets and importance
sums of oracle.evaluation_ref. A coefficient no cell displays is held: every mask keeps it. grad_wams
are an argument, so that the numbers ranked are those the device ranked.

The cell of every coefficient is found independently of wam_amd.frames: the slice assignments run on
bands whose values are their own band-major offsets ('native' frame: a canvas of the image's size).
"""
import numpy as np
import torch
from scipy.ndimage import gaussian_filter, zoom
from scipy.stats import spearmanr

from oracle import dwt
from oracle import evaluation_ref as E

BAR = 1e-4   # absolute, on class probabilities and scores
HELD = -1


def flat_bands(coeffs):
    return [coeffs[0]] + [b for lv in coeffs[1:] for b in lv]


def like_bands(flat, coeffs):
    out, o = [], 0
    for b in flat_bands(coeffs):
        out.append(flat[o:o + b.size].reshape(b.shape))
        o += b.size
    assert o == flat.size
    return [out[0]] + [tuple(out[1 + 3 * l:4 + 3 * l]) for l in range(len(coeffs) - 1)]


def coeff_cells(H, W, J, wavelet):
    """(cell int64 [K], (Hc, Wc)): the flat canvas cell that displays the coefficient at band-major offset
    k, or HELD. Bands are (A, then per level, coarsest first, horizontal 'da', vertical 'ad', diagonal
    'dd'), the order of oracle.dwt.wavedec2 and of the plan."""
    shapes = dwt.wavedec2(np.zeros((H, W)), wavelet, J, "symmetric")
    K = sum(b.size for b in flat_bands(shapes))
    idx = like_bands(np.arange(K, dtype=np.int64), shapes)
    canvas = np.full((H, W), -1, dtype=np.int64)
    a = idx[0]
    canvas[:a.shape[0], :a.shape[1]] = a
    for i, (h, v, d) in enumerate(idx[1:][::-1]):                # finest level first
        eh, sh = int(H / 2 ** i), int(H / 2 ** (i + 1))
        ew, sw = int(W / 2 ** i), int(W / 2 ** (i + 1))
        canvas[sh:eh, sw:ew] = d[:eh - sh, :ew - sw]
        canvas[sh:eh, :sw] = v[:eh - sh, :sw]
        canvas[:sh, sw:ew] = h[:sh, :ew - sw]
    cell = np.full(K, HELD, dtype=np.int64)
    shown = np.flatnonzero(canvas.reshape(-1) >= 0)
    ks = canvas.reshape(-1)[shown]
    assert np.unique(ks).size == ks.size, "a coefficient is displayed twice"
    cell[ks] = shown
    return cell, (H, W)


def mask_thr(n_iter, length):
    n_comp = int(length / n_iter)
    return [0] + [min(m * n_comp, length) for m in range(1, n_iter)] + [length]


def coeff_keeps(wam, cell, mode, n_iter):
    """[n_iter + 1, K] bool: the coefficients each mask keeps (stable tie order: the device's default)."""
    order = np.argsort(np.asarray(wam).reshape(-1), kind="stable")[::-1]
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    held = cell == HELD
    rk = rank[np.where(held, 0, cell)]
    return np.stack([held | ((rk < thr) != (mode == "deletion")) for thr in mask_thr(n_iter, order.size)])


def reconstruct(img, J, wavelet, factors):
    """img HWC float32 (show()), factors [M, K] float64 multipliers -> list of uint8 HWC images."""
    dec = [dwt.wavedec2(img[:, :, c].astype(np.float64), wavelet, J, "symmetric") for c in range(img.shape[2])]
    flat = [np.concatenate([b.reshape(-1) for b in flat_bands(d)]) for d in dec]
    out = []
    for f in factors:
        chans = [dwt.waverec2(like_bands(fl * f, d), wavelet) for fl, d in zip(flat, dec)]
        out.append((E.normalize_data(np.stack(chans, axis=2)) * 255).astype(np.uint8))
    return out


def evaluate_auc(model, grad_wams, x, y, mode, J, wavelet, n_iter):
    """-> (scores, curves); x [N, 3, H, W] tensor, model on the CPU."""
    scores, curves = [], []
    cell, _ = coeff_cells(x.shape[2], x.shape[3], J, wavelet)
    for s in range(x.shape[0]):
        alt = reconstruct(E.show(x[s]), J, wavelet, coeff_keeps(grad_wams[s], cell, mode, n_iter).astype(np.float64))
        with torch.no_grad():
            preds = model(torch.stack([E.to_input(im) for im in alt])).numpy()
        p = E.softmax_np(preds)[:, y[s]]
        scores.append(E.compute_auc(p))
        curves.append(p)
    return scores, curves


def _grid_factors(masks, hw, cell):
    """superpixel masks [n, g, g] zoomed (order 0) to the canvas -> [n, K] multipliers, 1.0 for held"""
    up = zoom(masks, (1, hw[0] / masks.shape[1], hw[1] / masks.shape[2]), order=0).reshape(masks.shape[0], -1)
    return np.where(cell[None, :] == HELD, 1.0, up[:, np.where(cell == HELD, 0, cell)])


def _probs(model, alt, label, batch_size):
    out = []
    for b in range(int(np.ceil(len(alt)) / batch_size)):  # the reference's (sic) batch count
        s, e = b * batch_size, min(len(alt), (b + 1) * batch_size)
        out.append(E.evaluate(torch.stack([E.to_input(im) for im in alt[s:e]]), label, model, batch_size).tolist())
    return np.array(sum(out, []))


def mu_fidelity(model, grad_wams, x, y, J, wavelet, grid_size, sample_size, subset_size, batch_size, random_seed=42):
    """oracle.evaluation_ref.mu_fidelity with the superpixel masks carried to the coefficients through the
    mosaic cells (the same draws from numpy's and Python's generators, in the same order)."""
    np.random.seed(random_seed)
    with torch.no_grad():
        base = E.softmax_np(model(x).numpy())
    cell, hw = coeff_cells(x.shape[2], x.shape[3], J, wavelet)
    out = []
    for i in range(len(grad_wams)):
        img = E.show(x[i])
        wam = gaussian_filter(grad_wams[i], sigma=2)
        indices = E.generate_subsets(grid_size, subset_size, sample_size)
        src = np.random.uniform(size=(sample_size, grid_size, grid_size))
        ys = _probs(model, reconstruct(img, J, wavelet, _grid_factors(src, hw, cell)), y[i], batch_size)
        bmask = src[np.argmin(ys), :, :]
        masks = np.ones((sample_size, grid_size, grid_size))
        for j, index_set in enumerate(indices):
            cx, cy = zip(*index_set)
            masks[j, cx, cy] = bmask[cx, cy]
        preds = base[i, y[i]] - _probs(model, reconstruct(img, J, wavelet, _grid_factors(masks, hw, cell)), y[i],
                                       batch_size)
        attrs = E.sum_importance(wam, indices, grid_size, sample_size, batch_size=batch_size)
        out.append(np.nanmean(spearmanr(preds, attrs)))
    return out
