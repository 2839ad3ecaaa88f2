"""Audio baselines on MI355X: the methods the audio WAM is compared against, and their evaluation.

Drop-in for the reference's ``EvalAudioBaselines`` (``src/evaluators.py:310-548``), the audio counterpart
of ``EvalImageBaselines``: Saliency, Integrated Gradients, SmoothGrad and Grad-CAM explain the model on
its own input, the dB mel spectrogram [N, 1, T, n_mels], and are scored with the measures ``Eval1DWAM``
gives the WAM's mel target. The explained model's forward and backward stay in PyTorch; everything around
them runs on the kernels the other evaluators use:

  waveforms --wam_melspec (the torch path where k_mel_fwd does not apply)--> source dB mel
  --Saliency / IntegratedGradients (wam_trapz_f32) / SmoothGrad (wam_item_sigma + wam_noise_add,
  wam_channel_mean) / GradCAM (wam_cam_maps, wam_cam_maps_tiled above its LDS bound: a full-resolution
  layer of 157 x 128 cells is past it)--> explanation [N, T, n_mels]
  --ranking of the signed explanation, wam_rank_mask_rows--> the n_iter + 1 masked spectrograms of several
  clips --model (no grad)--> host softmax, curves, AUC.

Host work left: the ranking's ``tie_order='numpy'`` option, the softmax and AUC on [n_iter + 1, classes]
logits.
"""
import numpy as np
import torch

from .baselines import GradCAM, IntegratedGradients, Saliency, SmoothGrad, _device_of, _targets
from .evalcore import check_tie_order, class_curves, compute_auc, db_melspec, rank_mask_rows
from .wam_1D import _peak_normalise as _peak_normalise_1d

AUDIO_METHODS = ("integratedgrad", "gradcam", "smoothgrad", "saliency")


class EvalAudioBaselines:
    """src/evaluators.py:310-548 -- insertion, deletion, faithfulness of spectra (Parekh et al.) and input
    fidelity (Paissan et al.) of an attribution method on the dB mel spectrogram, on the device. Same
    positional arguments, methods and return values.

    ``method_name``: 'integratedgrad', 'gradcam', 'smoothgrad', 'saliency'; any other name is a
    ValueError here, at construction (the reference constructs and fails later with an AttributeError on
    ``self.method``). ``layer``: Grad-CAM's target module; the default is ``model.layer``, which the
    reference hard-codes (a ValueError naming ``layer`` when the model has none). ``tie_order`` and
    ``eval_batch`` (model rows per forward, several clips' masks in one) as in Eval1DWAM.

    Explanations, numpy [N, T, n_mels]: Saliency and Integrated Gradients (riemann_trapezoid, 50 steps,
    ``batch_size`` rows per forward) are the attribution of the one mel channel, float32; SmoothGrad has
    the WAM's spread 0.001, 50 samples, seed 42 and returns float64 (its noise is the device Philox
    stream: the reference's torch.normal stream is unseeded, so there is none to reproduce); Grad-CAM is
    float32.

    Kept from the reference: the ranking is of the signed explanation; n_comp = int(P / n_iter) and the
    last mask is forced full; a dropped negative dB value becomes -0.0 -- masking sets dB cells to 0,
    which is loud: that is the reference's measure --; scores are np.float32 and curves float32 arrays;
    ``deletion()`` also overwrites ``insertion_curves`` (sic, :487; ``deletion_curves`` is set next to
    it); faithfulness_of_spectra is deletion with n_iter = 2, p[0] - p[1]; input_fidelity is the arg-max
    of rows 1 and 2 of insertion with n_iter = 2. With the reference's FtEx at clips short enough that
    ``model.layer`` yields a 1 x 1 map the CAM is 0 / 0 and the explanation NaN everywhere: the order a
    NaN explanation ranks in is not part of the contract, but it is a permutation, so rows 0 and n_iter
    are the empty and the full input.

    Not kept: ``explanations`` is honoured when a caller assigned it (as in EvalImageBaselines);
    otherwise explanations are computed per call and not stored, as in the reference."""

    def __init__(self, method_name, model, device=None, n_fft=1024, sample_rate=44100, n_mels=128, batch_size=64, *,
                 layer=None, tie_order="stable", eval_batch=520):
        if method_name not in AUDIO_METHODS:
            raise ValueError("EvalAudioBaselines: unknown method %r (one of %s)"
                             % (method_name, ", ".join(AUDIO_METHODS)))
        if method_name == "gradcam" and layer is None:
            layer = getattr(model, "layer", None)
            if layer is None:
                raise ValueError("EvalAudioBaselines: the model has no attribute 'layer' (the reference's Grad-CAM "
                                 "target); pass the target module as layer=")
        self.n_fft = n_fft
        self.n_mels = n_mels
        self.sample_rate = sample_rate
        self.batch_size = batch_size
        self.tie_order = check_tie_order(tie_order)
        self.eval_batch = eval_batch
        self.device = self._dev = _device_of(model, device)
        self.model = model
        self.method_name = method_name
        self.explanations = None
        self.insertion_curves = []
        self.deletion_curves = []
        if method_name == "integratedgrad":
            self.method = IntegratedGradients(model)
        elif method_name == "gradcam":
            self.method = GradCAM(model, layer)
        elif method_name == "smoothgrad":
            self.method = SmoothGrad(model, stdev_spread=0.001)  # same spread as the wam
        else:
            self.method = Saliency(model)

    # -------------------------------------------------------------------- device pipeline
    def _waves(self, x):
        if isinstance(x, list):
            x = _peak_normalise_1d(x)
        return torch.as_tensor(x).detach().to(self._dev, torch.float32).contiguous()

    def _mel(self, wave):
        with torch.no_grad():
            return db_melspec(wave, self.n_fft, self.sample_rate, self.n_mels)

    # -------------------------------------------------------------------- reference API
    def compute_explanations(self, x, y):
        """src/evaluators.py:353-392: the explanation on the mel spectrogram of x, numpy [N, T, n_mels]."""
        mel = self._mel(self._waves(x))
        if self.method_name == "integratedgrad":
            return self.method.attribute(mel, target=_targets(y, self._dev), method="riemann_trapezoid",
                                         return_convergence_delta=False, n_steps=50,
                                         internal_batch_size=self.batch_size).squeeze(1).detach().cpu().numpy()
        if self.method_name == "saliency":
            return self.method.attribute(mel, target=_targets(y, self._dev)).squeeze(1).detach().cpu().numpy()
        return self.method(mel, y)

    def auc_from_melspec(self, melspec, source_melspec, mode, n_iter):
        """src/evaluators.py:394-425 for one clip ([T, n_mels] explanation and dB mel spectrogram) or a
        batch of clips ([sets, T, n_mels]): [sets * (n_iter + 1), 1, T, n_mels] on the device."""
        return rank_mask_rows(melspec, source_melspec, n_iter, mode == "deletion", self._dev, self.tie_order)

    def evaluate_auc(self, x, y, mode, n_iter=64, argmax=False):
        """src/evaluators.py:427-475."""
        xd = self._waves(x)
        melspecs = self.explanations if self.explanations is not None else self.compute_explanations(xd, y)
        melspecs = np.asarray(melspecs)
        source = self._mel(xd)
        n_sounds = melspecs.shape[0]
        M = n_iter + 1
        scores, predicted_probs, raw_preds = [], [], []
        per_call = max(1, self.eval_batch // M)
        for s0 in range(0, n_sounds, per_call):
            group = list(range(s0, min(n_sounds, s0 + per_call)))
            inputs = self.auc_from_melspec(melspecs[group], source[group], mode, n_iter)
            with torch.no_grad():
                preds = self.model(inputs).float().cpu().numpy()
            raw_preds.extend(preds.reshape(len(group), M, -1))
            for prob in class_curves(preds, M, [y[s] for s in group]):
                scores.append(compute_auc(prob))
                predicted_probs.append(prob)
        if argmax:
            return raw_preds
        return scores, predicted_probs

    def insertion(self, x, y, n_iter):
        scores, predicted_probs = self.evaluate_auc(x, y, "insertion", n_iter)
        self.insertion_curves = predicted_probs
        return scores

    def deletion(self, x, y, n_iter):
        scores, predicted_probs = self.evaluate_auc(x, y, "deletion", n_iter)
        self.insertion_curves = predicted_probs  # sic (src/evaluators.py:487)
        self.deletion_curves = predicted_probs
        return scores

    def faithfulness_of_spectra(self, x, y):
        """src/evaluators.py:490-519: the drop of the class probability when the more important half of
        the cells is deleted (deletion with n_iter = 2, p[0] - p[1])."""
        _, predicted_probs = self.evaluate_auc(x, y, "deletion", 2)
        predicted_probs = np.array(predicted_probs)
        return (predicted_probs[:, 0] - predicted_probs[:, 1]).tolist()

    def input_fidelity(self, x, y):
        """src/evaluators.py:521-548: arg-max classes with the more important half and with all of the
        cells inserted (insertion with n_iter = 2, rows 1 and 2)."""
        preds = np.array(self.evaluate_auc(x, y, "insertion", 2, argmax=True))
        return np.argmax(preds[:, 1:, :], axis=2).tolist()
