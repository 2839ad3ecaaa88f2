"""Insertion and deletion for voxel WAMs on MI355X: ``Eval3DWAM``.

An addition: the reference evaluates images and audio (``src/evaluators.py``) and has no evaluator for
volumes. This is the metric of the other two modalities restated for ``WaveletAttribution3D``'s |grad|
cube with the project's own conventions: ``generate_masks``' threshold rule (mask m keeps the
m * int(S^3 / n_iter) most important cube voxels, the last mask everything), ``compute_auc``,
``tie_order`` and ``eval_batch`` as in ``Eval2DWAM`` / ``Eval1DWAM``, ``grad_wams`` computed once and
cached. Per group of volumes (``eval_batch // (n_iter + 1)`` volumes per model forward, at least one):

  wam_wavedec (the evaluator's ``mode``) --ranks of the cube values as given (signed) on the device-->
  wam_waverec_ranked (all n_iter + 1 masked reconstructions of every volume; on 3D Haar plans with
  J <= 2 the rank threshold is applied as the synthesis loads, nothing is stored in between)
  --> model (no grad) on the raw float reconstructions --> host softmax and AUC

Every cube voxel stands for one coefficient (``BaseWAM3D.refactor``'s packing, ``frames.cube_map``), so
masking the cube is masking the coefficients through the inverse of that map. The packing is such a
bijection only for a cubic volume whose band sizes sum to S^3 (Haar at sizes divisible by 2^J);
anything else is a ValueError. Out of scope: mu-fidelity (it needs a 3D superpixel grid) and
multi-channel volumes (``_check_channels`` refuses them, as the attribution does).
"""
import types

import numpy as np
import torch

from . import frames
from .evalcore import check_tie_order, class_curves, compute_auc, descending_ranks, device_table
from .plan import get_plan
from .wam_3D import WaveletAttribution3D


def cube_pos_table(S, levels, band_shapes):
    """The cube voxel (flat index into [S, S, S]) of every coefficient of a volume, int32
    [sum(band sizes)]: the inverse of frames.cube_map, on the host. ValueError unless the cube is a
    bijection onto the coefficients."""
    S = int(S)
    sizes = [int(np.prod(s)) for s in band_shapes]
    K = int(sum(sizes))
    what = ("Eval3DWAM needs the |grad| cube to be a bijection onto the coefficients: a cubic volume whose "
            "band sizes sum to S^3; J=%d at S=%d has %d coefficients for %d cube voxels" % (levels, S, K, S ** 3))
    if K != S ** 3:
        raise ValueError(what)
    plan = types.SimpleNamespace(levels=int(levels), band_shapes=[tuple(s) for s in band_shapes],
                                 band_offsets=np.concatenate([[0], np.cumsum(sizes)]).tolist())
    src = frames.cube_index(plan, S).reshape(-1)
    if (src < 0).any() or np.unique(src).size != K:
        raise ValueError(what)
    pos = np.empty(K, dtype=np.int32)
    pos[src] = np.arange(K, dtype=np.int32)
    return pos


class Eval3DWAM(WaveletAttribution3D):
    """Insertion / deletion (Petsiuk et al.), faithfulness and input fidelity of a voxel WAM, on the
    device. ``WaveletAttribution3D``'s positional arguments, then ``batch_size``; ``**wam_kw`` go to the
    inner ``WaveletAttribution3D`` that produces ``grad_wams`` (computed once and cached). Side
    attributes as the other evaluators: ``grad_wams``, ``insertion_curves``, ``deletion_curves``."""

    def __init__(self, model, wavelet="haar", J=3, approx_coeffs=False, device=None, mode="symmetric",
                 instance="voxels", method="smooth", normalize=True, EPS=0.451, n_samples=25, stdev_spread=0.0001,
                 random_seed=42, batch_size=128, *, tie_order="stable", eval_batch=520, **wam_kw):
        super().__init__(model, wavelet=wavelet, J=J, approx_coeffs=approx_coeffs, device=device, mode=mode,
                         instance=instance, method=method, normalize=normalize, EPS=EPS, n_samples=n_samples,
                         stdev_spread=stdev_spread, random_seed=random_seed)
        self.gradwam = WaveletAttribution3D(model, wavelet=wavelet, J=J, approx_coeffs=approx_coeffs, device=device,
                                            mode=mode, instance=instance, method=method, normalize=normalize, EPS=EPS,
                                            n_samples=n_samples, stdev_spread=stdev_spread, random_seed=random_seed,
                                            **wam_kw)
        self.batch_size = batch_size
        self.grad_wams = None
        self.tie_order = check_tie_order(tie_order)
        self.eval_batch = eval_batch
        self.insertion_curves = []
        self.deletion_curves = []

    def _pos(self, plan, S):
        return device_table(("cube_pos", plan, S, self._dev), lambda: torch.as_tensor(
            cube_pos_table(S, plan.levels, plan.band_shapes)).to(self._dev))

    def evaluate_auc(self, x, y, mode, n_iter=64, argmax=False):
        """AUC of the class probability along the insertion (deletion) path of the WAM ranking ->
        (scores, predicted_probs); argmax=True returns the raw logits [N, n_iter + 1, classes] instead."""
        if y is None:
            raise ValueError("Eval3DWAM needs the class labels y")
        if self.grad_wams is None:
            self.grad_wams = self.gradwam(x, y)
        dev = self._dev
        xd = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
        if xd.dim() != 5:
            raise ValueError("x must be [N, 1, S, S, S], got %s" % (tuple(xd.shape),))
        n, c = xd.shape[:2]
        sp = tuple(xd.shape[2:])
        S = sp[-1]
        plan = get_plan(3, sp, self.J, self.wavelet, self.mode, dev)
        self._check_channels(c, plan.band_shapes[0][0])
        if sp != (S, S, S):
            raise ValueError("Eval3DWAM needs the |grad| cube to be a bijection onto the coefficients: a cubic "
                             "volume whose band sizes sum to S^3; got a volume of %s" % (sp,))
        pos = self._pos(plan, S)
        cube = np.reshape(np.asarray(self.grad_wams), (n, -1))
        M = n_iter + 1
        per_call = max(1, self.eval_batch // M)
        scores, predicted_probs, raw_preds = [], [], []
        for s0 in range(0, n, per_call):
            group = list(range(s0, min(n, s0 + per_call)))
            coeffs = plan.wavedec(xd[group].view((len(group),) + sp))
            rank = descending_ranks(cube[group], dev, self.tie_order)
            rec = plan.waverec_ranked(coeffs, len(group), rank, pos, n_iter, int(S ** 3 / n_iter), mode == "deletion")
            with torch.no_grad():
                preds = self.model(rec.view((len(group) * M, 1) + plan.rec_shape)).float().cpu().numpy()
            raw_preds.extend(preds.reshape(len(group), M, -1))
            for p in class_curves(preds, M, [y[s] for s in group]):
                scores.append(compute_auc(p))
                predicted_probs.append(p)
        if argmax:
            return raw_preds
        return scores, predicted_probs

    def insertion(self, x, y, n_iter=64):
        scores, predicted_probs = self.evaluate_auc(x, y, "insertion", n_iter=n_iter)
        self.insertion_curves = predicted_probs
        return scores

    def deletion(self, x, y, n_iter=64):
        scores, predicted_probs = self.evaluate_auc(x, y, "deletion", n_iter=n_iter)
        self.deletion_curves = predicted_probs
        return scores

    def faithfulness(self, x, y):
        """The drop of the class probability when the more important half of the coefficients is
        deleted (deletion with n_iter = 2, p[0] - p[1]), as Eval1DWAM.faithfulness_of_spectra."""
        _, predicted_probs = self.evaluate_auc(x, y, "deletion", 2)
        predicted_probs = np.array(predicted_probs)
        return (predicted_probs[:, 0] - predicted_probs[:, 1]).tolist()

    def input_fidelity(self, x, y):
        """Arg-max classes with the more important half and with all of the coefficients inserted
        (insertion with n_iter = 2, rows 1 and 2), as Eval1DWAM.input_fidelity."""
        preds = np.array(self.evaluate_auc(x, y, "insertion", 2, argmax=True))
        return np.argmax(preds[:, 1:, :], axis=2).tolist()
