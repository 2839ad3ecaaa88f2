"""Plain-numpy restatement of the reference's EvalAudioBaselines (src/evaluators.py:310-548) (TEST
INFRASTRUCTURE).

It follows the class line by line on a CPU model: compute_melspec (oracle.melspec per waveform), the
method on the mel input, generate_masks' float64 masks times the source spectrogram, a float32 cast, the
model, the host softmax and compute_auc. The methods are those of tests/baselines_ref.py (saliency_ref's
input gradients, integrated_gradients_ref, smoothgrad_ref, gradcam_ref -- float64 where the reference's
Grad-CAM is float32: D_CAM), the front-end and the masks those of tests/eval1d_ref.py. ``sort='stable'``
ranks ties as the device does by default (a stable ascending sort, reversed) where ``'numpy'`` is the
reference's np.argsort.
"""
import numpy as np
import torch

from tests import baselines_ref as B
from tests import eval1d_ref as R1

F32, F64 = np.float32, np.float64
METHODS = ("integratedgrad", "gradcam", "smoothgrad", "saliency")


def peak_normalise(x):
    return torch.tensor(np.array([wf / wf.max() for wf in x]).astype(F32))


def source_melspec(x, cfg):
    """compute_melspec: [N, 1, T, n_mels] float32 torch."""
    if isinstance(x, list):
        x = peak_normalise(x)
    return R1.compute_melspec(x, cfg["n_fft"], cfg["sample_rate"], cfg["n_mels"])


def compute_explanations(model, method, x, y, cfg, layer=None, noisy=None):
    """compute_explanations (:353-392) -> numpy [N, T, n_mels]. ``noisy``: SmoothGrad's noisy inputs
    [n_samples, N, 1, T, n_mels] (the reference draws them from an unseeded stream)."""
    mel = source_melspec(x, cfg)
    if method == "saliency":
        return np.abs(B.input_grads(model, mel, y)).squeeze(1)
    if method == "integratedgrad":
        return B.integrated_gradients_ref(model, mel, y, n_steps=50).squeeze(1).astype(F32)
    if method == "gradcam":
        return B.gradcam_ref(model, model.layer if layer is None else layer, mel, y)
    if method == "smoothgrad":
        return B.smoothgrad_ref(model, mel, y, noisy)
    raise AttributeError("'EvalAudioBaselines' object has no attribute 'method'")


def descending_order(values, sort="numpy"):
    v = np.asarray(values).reshape(-1)
    return (np.argsort(v, kind="stable") if sort == "stable" else np.argsort(v, axis=None))[::-1]


def rank_of(order):
    rank = np.empty(order.size, dtype=np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32)
    return rank


def melspec_inputs(expl, source, mode, n_iter, sort="numpy"):
    """auc_from_melspec (:394-425) with generate_masks (src/evaluation_helpers.py:455-499):
    [n_iter + 1, 1, T, n_mels] float32 torch."""
    ins = R1.insertion_masks(descending_order(expl, sort), n_iter).reshape((n_iter + 1,) + expl.shape)
    return torch.tensor((1.0 - ins if mode == "deletion" else ins) * source).float().unsqueeze(1)


def evaluate_auc(model, expl, x, y, mode, n_iter, cfg, sort="numpy", keep=None):
    """evaluate_auc (:427-475) on given explanations -> (scores, curves, raw logits); keep: a list that
    receives the model inputs per clip."""
    source = source_melspec(x, cfg).squeeze(1).numpy()
    scores, curves, raw = [], [], []
    for s in range(expl.shape[0]):
        inputs = melspec_inputs(expl[s], source[s], mode, n_iter, sort)
        with torch.no_grad():
            preds = model(inputs).cpu().numpy()
        probs = np.exp(preds) / np.sum(np.exp(preds), axis=1, keepdims=True)
        p = probs[:, y[s]]
        scores.append(R1.compute_auc(p))
        curves.append(p)
        raw.append(preds)
        if keep is not None:
            keep.append(inputs.numpy())
    return scores, curves, raw


def faithfulness_of_spectra(model, expl, x, y, cfg, sort="numpy"):
    curves = np.array(evaluate_auc(model, expl, x, y, "deletion", 2, cfg, sort)[1])
    return (curves[:, 0] - curves[:, 1]).tolist()


def input_fidelity(model, expl, x, y, cfg, sort="numpy"):
    raw = evaluate_auc(model, expl, x, y, "insertion", 2, cfg, sort)[2]
    return np.argmax(np.array(raw)[:, 1:, :], axis=2).tolist()
