"""Insertion, deletion and mu-fidelity for voxel WAMs on MI355X: ``Eval3DWAM``.

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
anything else is a ValueError. Out of scope: multi-channel volumes (``_check_channels`` refuses them, as
the attribution does).

``mu_fidelity`` (Bhatt et al.) is the image evaluator's metric on a grid_size^3 superpixel grid: the
float-valued grid masks reach the coefficients through cube voxel -> grid cell (scipy's order-0 zoom of
the cell indices, ``evalcore.zoom_cell_map3``), and per group of volumes

  wam_wavedec --> wam_waverec_cells (the sample_size reconstructions of every volume under its own masks;
  on 3D Haar plans with J <= 2 the mask rows are staged in LDS and multiply the coefficients as the
  synthesis loads them) --> model (no grad) --> host softmax

runs twice: for the baseline-state search and for the subsets. The attribution is smoothed by
wam_gaussian_filter3d (scipy's ``gaussian_filter`` in bits) and summed over each subset's voxels by
wam_masked_sums; Spearman's rho of the probability drops against the sums is the score.
"""
import random
import types
import warnings

import numpy as np
import torch
from scipy.stats import spearmanr

from . import frames
from .evalcore import (cell_map3, check_tie_order, class_curves, compute_auc, descending_ranks, device_table,
                       gaussian_weights, masked_sums, softmax)
from .plan import gaussian_filter3d, get_plan
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
    """Insertion / deletion (Petsiuk et al.), faithfulness, input fidelity and mu-fidelity (Bhatt et al.)
    of a voxel WAM, on the device. ``WaveletAttribution3D``'s positional arguments, then ``batch_size``;
    ``**wam_kw`` go to the inner ``WaveletAttribution3D`` that produces ``grad_wams`` (computed once and
    cached). Side attributes as the other evaluators: ``grad_wams``, ``insertion_curves``,
    ``deletion_curves``; ``mu_details`` after ``mu_fidelity``. ``cells_route``: wam_waverec_cells' route in
    ``mu_fidelity``, -1 = the plan's own (0 / 1 force one)."""

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
        self.cells_route = -1
        self.mu_details = []

    def _pos(self, plan, S):
        return device_table(("cube_pos", plan, S, self._dev), lambda: torch.as_tensor(
            cube_pos_table(S, plan.levels, plan.band_shapes)).to(self._dev))

    def _checked(self, x, y):
        """The checks every method starts with -- labels present, grad_wams computed once, x [N, 1, S, S, S]
        cubic, the cube a bijection onto the coefficients -> (x on the device, N, S, plan, cube-voxel table)."""
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
        return xd, n, S, plan, self._pos(plan, S)

    def evaluate_auc(self, x, y, mode, n_iter=64, argmax=False):
        """AUC of the class probability along the insertion (deletion) path of the WAM ranking ->
        (scores, predicted_probs); argmax=True returns the raw logits [N, n_iter + 1, classes] instead."""
        xd, n, S, plan, pos = self._checked(x, y)
        sp = plan.shape
        dev = self._dev
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

    # ---------------------------------------------------------------------------------- mu-fidelity
    def _slot(self, plan, S, grid_size, pos):
        """The grid cell of every coefficient, int32 [K] on the device: cell[pos[k]], cached per plan, S and
        grid."""
        return device_table(("cells_slot", plan, S, int(grid_size), self._dev), lambda: cell_map3(
            grid_size, S, self._dev)[pos.long()].contiguous())

    def _masked_probs(self, plan, coeffs, group, slot, grids, labels):
        """Class probabilities of the volumes of `group` (their coefficients in `coeffs`) reconstructed
        under their own masks grids [len(group), n_masks, G] (host float32): one wam_waverec_cells call, the
        model on the raw float reconstructions at most eval_batch rows per forward -> [len(group), n_masks]."""
        n_masks = grids.shape[1]
        gd = torch.as_tensor(np.ascontiguousarray(grids, dtype=np.float32)).to(self._dev)
        rec = plan.waverec_cells(coeffs, len(group), slot, gd, route=self.cells_route)
        rec = rec.view((len(group) * n_masks, 1) + plan.rec_shape)
        step = max(1, int(self.eval_batch))
        with torch.no_grad():
            preds = np.concatenate([softmax(self.model(rec[r0:r0 + step]).float().cpu().numpy())
                                    for r0 in range(0, rec.shape[0], step)])
        return np.stack([preds[k * n_masks:(k + 1) * n_masks, label] for k, label in enumerate(labels)])

    def compute_baseline_state(self, volume, label, grid_size=8, sample_size=128, source=None):
        """The uniform random superpixel mask [grid_size] * 3 whose reconstruction of `volume` ([S, S, S] or
        [1, S, S, S]) has the lowest probability of `label`: source[argmin]. source [sample_size, g, g, g]
        float32: the candidates; None draws them as mu_fidelity draws its first volume's, from
        np.random.RandomState(random_seed) (the global numpy state is not touched)."""
        dev = self._dev
        xd = torch.as_tensor(volume).detach().to(dev, torch.float32).contiguous()
        S = int(xd.shape[-1])
        if xd.numel() != S ** 3:
            raise ValueError("compute_baseline_state takes one cubic single-channel volume, got %s" % (tuple(xd.shape),))
        plan = get_plan(3, (S, S, S), self.J, self.wavelet, self.mode, dev)
        slot = self._slot(plan, S, grid_size, self._pos(plan, S))
        if source is None:
            source = np.random.RandomState(self.random_seed).uniform(
                size=(sample_size,) + (grid_size,) * 3).astype(np.float32)
        source = np.asarray(source, dtype=np.float32)
        pb = self._masked_probs(plan, plan.wavedec(xd.view(1, S, S, S)), [0], slot,
                                source.reshape(1, source.shape[0], -1), [label])[0]
        return source[int(np.argmin(pb))]

    def mu_fidelity(self, x, y, grid_size=8, sample_size=128, subset_size=None, sigma=2.0):
        """mu-fidelity (Bhatt et al.) of the voxel WAM on a grid_size^3 superpixel grid -> [N] floats.
        Per volume: the baseline state is the one of sample_size uniform random grid masks whose masked
        reconstruction has the lowest class probability; each of sample_size random subsets of subset_size
        cells (None: int(0.2 * grid_size^3)) sets its cells to the baseline state's values, all other cells
        to 1; the score is Spearman's rho between the drops of the class probability and the sums of the
        Gaussian-smoothed (sigma; <= 0: not smoothed) attribution over each subset's voxels, NaN when
        either is constant. This is rho alone, the paper's definition: Eval2DWAM and the image baselines
        average rho with its p-value because the reference does.
        Draws: random.Random(random_seed) for the subsets and np.random.RandomState(random_seed) for the
        candidate masks, fresh at every call, per volume in order (subsets, then candidates); the global
        random and numpy states are neither read nor changed. ``mu_details``: per volume a dict of
        baseline_index, baseline_probs [sample_size], altered_probs [sample_size], sums [sample_size]
        (float64) and base_prob."""
        xd, n, S, plan, pos = self._checked(x, y)
        g = int(grid_size)
        if g < 1 or g > S:
            raise ValueError("grid_size must be in 1..S = %d, got %d" % (S, g))
        G = g ** 3
        subset_size = int(0.2 * G) if subset_size is None else int(subset_size)
        if sample_size < 1 or not 1 <= subset_size <= G:
            raise ValueError("sample_size >= 1 and 1 <= subset_size <= %d, got %d and %d" % (G, sample_size, subset_size))
        dev = self._dev
        cell = cell_map3(g, S, dev)
        slot = self._slot(plan, S, g, pos)
        pr, rs = random.Random(self.random_seed), np.random.RandomState(self.random_seed)
        subsets, sources = [], []
        for _ in range(n):
            subsets.append([pr.sample(range(G), subset_size) for _ in range(sample_size)])
            sources.append(rs.uniform(size=(sample_size, g, g, g)).astype(np.float32))
        with torch.no_grad():
            base = softmax(self.model(xd).float().cpu().numpy())
        wts, radius = gaussian_weights(sigma) if sigma > 0 else (None, 0)
        per_call = max(1, int(self.eval_batch) // sample_size)
        mu, details = [], []
        for s0 in range(0, n, per_call):
            group = list(range(s0, min(n, s0 + per_call)))
            labels = [y[i] for i in group]
            coeffs = plan.wavedec(xd[group].view((len(group), S, S, S)))
            pbs = self._masked_probs(plan, coeffs, group, slot,
                                     np.stack([sources[i].reshape(sample_size, G) for i in group]), labels)
            masks = np.ones((len(group), sample_size, G), dtype=np.float32)
            for k, i in enumerate(group):
                bmask = sources[i][int(np.argmin(pbs[k]))].reshape(-1)
                for j, sub in enumerate(subsets[i]):
                    masks[k, j, sub] = bmask[sub]
            alts = self._masked_probs(plan, coeffs, group, slot, masks, labels)
            for k, i in enumerate(group):
                wam = torch.as_tensor(np.ascontiguousarray(self.grad_wams[i], dtype=np.float64)).to(dev).view(S, S, S)
                if wts is not None:
                    wam = gaussian_filter3d(wam, wts, radius)
                sub = np.zeros((sample_size, G), dtype=np.float32)
                for j, idx in enumerate(subsets[i]):
                    sub[j, idx] = 1
                sums = masked_sums(wam.reshape(-1), sub, cell)
                preds = np.float64(base[i, y[i]]) - alts[k].astype(np.float64)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # a constant input: rho is NaN, which is the answer
                    mu.append(float(spearmanr(preds, sums).statistic))
                details.append({"baseline_index": int(np.argmin(pbs[k])), "baseline_probs": pbs[k],
                                "altered_probs": alts[k], "sums": sums, "base_prob": base[i, y[i]]})
        self.mu_details = details
        return mu
