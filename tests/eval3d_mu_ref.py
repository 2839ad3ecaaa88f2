"""Plain-numpy float64 restatement of wam_amd.evaluation3d.Eval3DWAM.mu_fidelity (TEST INFRASTRUCTURE).

Built on tests/eval3d_ref.py (coeff_voxels, flat_bands, like_bands), float64 oracle.dwt.wavedec3 /
waverec3, scipy's zoom and gaussian_filter and testmodels.TinyVoxel on the CPU. It follows the draw
protocol the method documents -- random.Random(seed) for the subsets, np.random.RandomState(seed) for the
candidate masks, per volume in order, subsets first -- and touches no global random state. It takes
grad_wams as an argument (it scores the numbers the device scored) and, optionally, a baseline_index per
volume: the probabilities of two candidate masks can lie closer than the device's error on a probability,
so the device's choice is handed over and judged separately.

Nothing here goes through a cell map: the float masks themselves are zoomed to the cube
(scipy.ndimage.zoom, order 0) and carried to the coefficients by the cube packing.
"""
import math
import random

import numpy as np
import torch
from scipy.ndimage import gaussian_filter, zoom
from scipy.stats import spearmanr

from oracle import dwt
from tests import eval3d_ref as R
from tests.eval3d_ref import BAR, softmax  # noqa: F401


def upsample(masks, S):
    """[n, g, g, g] float masks -> [n, S, S, S]: scipy's order-0 zoom of the masks themselves."""
    masks = np.asarray(masks)
    g = masks.shape[1]
    out = zoom(masks, (1,) + (S / g,) * 3, order=0)
    assert out.shape == (masks.shape[0], S, S, S), out.shape
    return out


def draws(seed, n, g, sample_size, subset_size):
    """(subsets, sources) of n volumes: subsets[i] = sample_size lists of subset_size cells (C order),
    sources[i] [sample_size, g, g, g] float32."""
    pr, rs = random.Random(seed), np.random.RandomState(seed)
    subsets, sources = [], []
    for _ in range(n):
        subsets.append([pr.sample(range(g ** 3), subset_size) for _ in range(sample_size)])
        sources.append(rs.uniform(size=(sample_size, g, g, g)).astype(np.float32))
    return subsets, sources


def masked_recs(x_s, masks, J, wavelet="haar", bmode="symmetric"):
    """The float64 reconstructions [n, S, S, S] of one volume under float masks [n, g, g, g]: every
    coefficient times the zoomed mask's value at its cube voxel."""
    S = x_s.shape[-1]
    coeffs = dwt.wavedec3(np.asarray(x_s, dtype=np.float64), wavelet, J, bmode)
    flat = np.concatenate([b.reshape(-1) for b in R.flat_bands(coeffs)])
    vox = R.coeff_voxels(S, J, wavelet, bmode)
    up = upsample(np.asarray(masks, dtype=np.float64), S).reshape(len(masks), -1)
    return np.stack([dwt.waverec3(R.like_bands(flat * u[vox], coeffs), wavelet) for u in up])


def class_probs(model, rec, label):
    with torch.no_grad():
        return softmax(model(torch.as_tensor(rec.astype(np.float32)).unsqueeze(1)).numpy())[:, label]


def mu_fidelity(model, x, y, grad_wams, J, grid_size, sample_size, subset_size=None, sigma=2.0, seed=42,
                baseline_index=None, wavelet="haar", bmode="symmetric"):
    """-> per volume a dict: mu, baseline_index, baseline_probs, altered_probs, sums, sum_mags (the sum
    of the magnitudes behind each of `sums`, for the summation bound), base_prob, source, subsets."""
    x = np.asarray(x, dtype=np.float32)
    n, S, g = x.shape[0], x.shape[-1], int(grid_size)
    G = g ** 3
    subset_size = int(0.2 * G) if subset_size is None else subset_size
    subsets, sources = draws(seed, n, g, sample_size, subset_size)
    with torch.no_grad():
        base = softmax(model(torch.as_tensor(x)).numpy())
    out = []
    for i in range(n):
        pb = class_probs(model, masked_recs(x[i, 0], sources[i], J, wavelet, bmode), y[i])
        b = int(np.argmin(pb)) if baseline_index is None else int(baseline_index[i])
        bmask = sources[i][b].reshape(-1)
        masks = np.ones((sample_size, G), dtype=np.float32)
        sub = np.zeros((sample_size, G), dtype=np.float32)
        for j, idx in enumerate(subsets[i]):
            masks[j, idx] = bmask[idx]
            sub[j, idx] = 1
        alt = class_probs(model, masked_recs(x[i, 0], masks.reshape(sample_size, g, g, g), J, wavelet, bmode), y[i])
        wam = np.asarray(grad_wams[i], dtype=np.float64)
        if sigma > 0:
            wam = gaussian_filter(wam, sigma)
        terms = wam.reshape(1, -1) * upsample(sub.reshape(sample_size, g, g, g).astype(np.float64), S).reshape(sample_size, -1)
        sums = np.array([math.fsum(t) for t in terms])
        mags = np.array([math.fsum(np.abs(t)) for t in terms])
        preds = np.float64(base[i, y[i]]) - alt.astype(np.float64)
        out.append({"mu": float(spearmanr(preds, sums).statistic), "baseline_index": b, "baseline_probs": pb,
                    "altered_probs": alt, "sums": sums, "sum_mags": mags, "base_prob": base[i, y[i]],
                    "source": sources[i], "subsets": subsets[i]})
    return out
