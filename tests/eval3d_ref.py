"""Plain-numpy float64 restatement of wam_amd.evaluation3d.Eval3DWAM (TEST INFRASTRUCTURE).

The reference has no evaluator for volumes, so this restates the definition the class documents, from
the parts the reference does have: generate_masks' threshold rule on the |grad| cube
(thr(m) = m * int(S^3 / n_iter), the last mask forced full), the cube packing of
oracle.wam_ref.refactor_3d (BaseWAM3D.refactor) to carry a cube mask to the coefficients, float64
oracle.dwt.wavedec3 / waverec3, testmodels.TinyVoxel on the CPU, the host softmax and compute_auc.
It takes grad_wams as an argument, so that it ranks the numbers the device ranked.

The coefficient of every cube voxel is found independently of wam_amd.frames: refactor_3d is run on
coefficients whose values are their own band-major index.
"""
import numpy as np
import torch

from oracle import dwt
from oracle.wam_ref import refactor_3d
from tests.eval1d_ref import BAR  # noqa: F401  (1e-4 absolute on class probabilities: the 2D evaluator's bar)

KEYS3 = dwt.KEYS3


def descending_order(values):
    """The device's default tie rule ('stable'): a stable ascending sort, reversed."""
    return np.argsort(np.asarray(values).reshape(-1), kind="stable")[::-1]


def mask_thr(n_iter, length):
    """thr(0) = 0, thr(m) = min(m * n_comp, length) for 0 < m < n_iter, thr(n_iter) = length."""
    n_comp = int(length / n_iter)
    return [0] + [min(m * n_comp, length) for m in range(1, n_iter)] + [length]


def flat_bands(coeffs):
    return [coeffs[0]] + [lv[k] for lv in coeffs[1:] for k in KEYS3]


def like_bands(flat, coeffs):
    """A flat band-major vector in the container layout of `coeffs`."""
    out, o = [], 0
    for b in flat_bands(coeffs):
        out.append(flat[o:o + b.size].reshape(b.shape))
        o += b.size
    assert o == flat.size
    return [out[0]] + [dict(zip(KEYS3, out[1 + 7 * l:8 + 7 * l])) for l in range(len(coeffs) - 1)]


def coeff_voxels(S, J, wavelet="haar", mode="symmetric"):
    """int64 [K]: the flat cube voxel of the coefficient at band-major offset k, from refactor_3d run on
    index-valued coefficients (k + 1: |.| leaves it alone and float32 holds it exactly below 2^24)."""
    shapes = dwt.wavedec3(np.zeros((S, S, S)), wavelet, J, mode)
    K = sum(b.size for b in flat_bands(shapes))
    assert K < 2 ** 24
    cube = refactor_3d([like_bands(np.arange(1, K + 1, dtype=np.float64), shapes)], J, S)[0].reshape(-1)
    ids = np.rint(cube).astype(np.int64) - 1
    assert K == S ** 3 and np.array_equal(np.sort(ids), np.arange(K)), "the cube is no bijection onto the coefficients"
    vox = np.empty(K, dtype=np.int64)
    vox[ids] = np.arange(S ** 3)
    return vox


def masked_sets(x_s, cube_s, mode, n_iter, J, wavelet="haar", bmode="symmetric"):
    """The n_iter + 1 masked coefficient containers (float64) of one volume x_s [S, S, S]."""
    S = x_s.shape[-1]
    coeffs = dwt.wavedec3(np.asarray(x_s, dtype=np.float64), wavelet, J, bmode)
    flat = np.concatenate([b.reshape(-1) for b in flat_bands(coeffs)])
    order = descending_order(cube_s)
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    rank_of_coeff = rank[coeff_voxels(S, J, wavelet, bmode)]
    out = []
    for thr in mask_thr(n_iter, S ** 3):
        keep = (rank_of_coeff < thr) != (mode == "deletion")
        out.append(like_bands(flat * keep, coeffs))
    return out


def softmax(preds):
    return np.exp(preds) / np.sum(np.exp(preds), axis=1, keepdims=True)


def compute_auc(probs):
    return sum(probs) / (np.max(probs) * len(probs))


def evaluate_auc(model, x, y, grad_wams, mode, n_iter, J, wavelet="haar", bmode="symmetric"):
    """-> (scores, curves, raw logits) per volume; x [N, 1, S, S, S], model on the CPU."""
    x = np.asarray(x, dtype=np.float32)
    scores, curves, raw = [], [], []
    for s in range(x.shape[0]):
        rec = np.stack([dwt.waverec3(c, wavelet) for c in masked_sets(x[s, 0], grad_wams[s], mode, n_iter, J, wavelet,
                                                                      bmode)])
        with torch.no_grad():
            preds = model(torch.as_tensor(rec.astype(np.float32)).unsqueeze(1)).numpy()
        p = softmax(preds)[:, y[s]]
        scores.append(compute_auc(p))
        curves.append(p)
        raw.append(preds)
    return scores, curves, raw


def faithfulness(model, x, y, grad_wams, J, wavelet="haar", bmode="symmetric"):
    curves = np.array(evaluate_auc(model, x, y, grad_wams, "deletion", 2, J, wavelet, bmode)[1])
    return (curves[:, 0] - curves[:, 1]).tolist()


def input_fidelity(model, x, y, grad_wams, J, wavelet="haar", bmode="symmetric"):
    raw = np.array(evaluate_auc(model, x, y, grad_wams, "insertion", 2, J, wavelet, bmode)[2])
    return np.argmax(raw[:, 1:, :], axis=2).tolist()
