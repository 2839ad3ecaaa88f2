"""Wavelet-domain insertion, deletion and mu-fidelity on MI355X.

Drop-in for the reference's ``Eval2DWAM`` (``src/evaluators.py:553-801``) and the helpers it
calls (``src/evaluation_helpers.py:361-594``): same class, constructor arguments, methods,
return values and debug attributes (``insertion_curves``, ``deletion_curves``, ``grad_wams``).
The reference reconstructs every altered image on the CPU, mask by mask and channel by channel
(pywt.wavedec2 -> coeffs_to_array -> arr * mask -> array_to_coeffs -> waverec2), round-trips it
through uint8 / PIL, and runs the model on the result. Here, per image:

  show()-normalised planes --wam_wavedec (pywt's default mode 'symmetric')--> coefficients
  --wam_coeff_masks (all masks x 3 channels, pywt coeffs_to_array positions)--> band-major
  --wam_waverec (one launch)--> reconstructions --wam_quantize_normalize (min-max, uint8
  truncation, ToTensor, ImageNet Normalize)--> model inputs on the device

and the model evaluates several images' masks per forward. Insertion / deletion masks come from
the importance ranking (wam_rank_masks); mu-fidelity's superpixel masks are upsampled through
scipy.ndimage.zoom's order-0 cell map (wam_upsample_masks), its Gaussian-smoothed importance and
subset sums are wam_gaussian_filter2d / wam_masked_sums. Host work left: the ranking's tie order
option, Python/numpy RNG draws (the reference's own streams), the softmax on [M, classes]
logits and spearmanr on sample_size values.

Semantics kept from the reference (pinned by tests/golden/eval_goldens.npz, made with the real
PyWavelets 1.1.1): the mask is applied in pywt's coeffs_to_array layout (cH bottom-left, cV
top-right -- transposed relative to the WAM mosaic), so the mask shape must equal the
coefficient array's (a ValueError as numpy's broadcast otherwise: haar at 224 is 224 x 224);
grad_wams are computed once and cached across calls; mu-fidelity seeds numpy with the INHERITED
random_seed (42) and averages spearmanr's (rho, p-value) pair; its batch count is
int(ceil(len) / batch_size) (sic). Tie order of equal importances: numpy's argsort is not
stable and differs across numpy builds; the default ranks ties stably (``tie_order='stable'``,
GPU), ``tie_order='numpy'`` ranks on the host with np.argsort like the reference.

``mask_layout="mosaic"`` (an addition, opt-in; the default ``"pywt"`` is the path above) scores every
coefficient by the WAM cell that displays it, for any wavelet and size the explainer can draw:
pos[k] = the mosaic cell of coefficient k (frames.wam_cell_source), the ranking is that of the WAM's
cells, n_comp = int(Hc * Wc / n_iter), and a coefficient no cell displays (the cropped border rows and
columns of non-Haar bands, approximation cells a detail block overwrote) is held: every insertion and
every deletion mask keeps it. Insertion's last and deletion's first image are therefore the exact
reconstruction, the other end the reconstruction of the held coefficients alone. One
wam_waverec2_ranked call serves a group of images (the float masks are never stored); mu-fidelity
keeps wam_coeff_masks, its superpixel grid zoomed to the WAM canvas.
Transform: the default (Resize((224, 224)) -- a no-op for 224 x 224 reconstructions --, ToTensor,
Normalize(ImageNet)) runs fused on the GPU; a user ``transform`` (a callable on HWC uint8 numpy
images) is applied on the host instead.

The audio evaluator ``Eval1DWAM`` (``src/evaluators.py:39-306``: insertion / deletion on wavelet
coefficients or the mel spectrogram, faithfulness of spectra, input fidelity) closes the module.
"""
import ctypes

import numpy as np
import torch
from scipy.stats import spearmanr

from ._lib import check, lib, ptr, stream_of
from .baselines import EvalImageBaselines  # noqa: F401  (the reference keeps it in this module)
from .baselines_audio import EvalAudioBaselines  # noqa: F401  (likewise)
from .evalcore import (IMAGENET_MEAN, IMAGENET_STD, array_layout, cell_map, check_tie_order,  # noqa: F401
                       class_curves, class_probs, coeff_array_layout, compute_auc, db_melspec, descending_ranks,
                       device_table, gaussian_weights, generate_subsets, masked_sums, norm_consts,
                       pil_bilinear_coeffs, rank_mask_rows, resize_default, show_images, softmax, zoom_cell_map)
from .evaluation3d import Eval3DWAM  # noqa: F401  (the volume evaluator, an addition: its own module)
from .frames import wam_cell_source
from .plan import get_plan, peak_divide
from .wam_1D import WaveletAttribution1D
from .wam_1D import _peak_normalise as _peak_normalise_1d
from .wam_2D import WaveletAttribution2D


class Eval2DWAM(WaveletAttribution2D):
    """src/evaluators.py:553-801 -- insertion / deletion (Petsiuk et al.), mu-fidelity (Bhatt et al.)."""

    def __init__(self, model, wavelet="haar", J=3, device=None, mode="reflect", transform=None, approx_coeffs=False,
                 method="smooth", n_samples=25, batch_size=128, stdev_spread=0.25, random_seed=42, *,
                 tie_order="stable", eval_batch=520, mask_layout="pywt", **wam_kw):
        super().__init__(model, wavelet=wavelet, J=J, device=device, mode=mode, approx_coeffs=approx_coeffs)
        if mask_layout not in ("pywt", "mosaic"):
            raise ValueError("mask_layout must be 'pywt' or 'mosaic', got %r" % (mask_layout,))
        self.mask_layout = mask_layout
        self.ranked_route = -1  # 'mosaic': wam_waverec2_ranked's route, -1 = the plan's own (0 / 1 force one)
        self.smooted_grad_wam = WaveletAttribution2D(model, wavelet=wavelet, J=J, mode=mode,
                                                     approx_coeffs=approx_coeffs, n_samples=n_samples,
                                                     stdev_spread=stdev_spread, random_seed=random_seed,
                                                     method=method, device=device, **wam_kw)
        self.batch_size = batch_size
        self.grad_wams = None
        self.transform = transform
        self.tie_order = check_tie_order(tie_order)
        self.eval_batch = eval_batch
        self.insertion_curves = []
        self.deletion_curves = []

    # -------------------------------------------------------------------- device pipeline
    def _images(self, x):
        return show_images(x, self._dev)

    def _layout(self, plan):
        return array_layout(plan, self._dev)

    def _mosaic_layout(self, plan):
        """mask_layout='mosaic': (pos int32 [K] on the device, the WAM canvas (Hc, Wc), the number of
        held coefficients) of the evaluation plan. pos[k] = the cell that displays coefficient k, or
        Hc * Wc -- the extra slot of the ranking -- for a coefficient no cell displays."""
        dev = self._dev
        wam = self.smooted_grad_wam

        def make():
            xplan = get_plan(2, plan.shape, self.J, self.wavelet, wam.mode, dev)  # the explainer's
            if list(xplan.band_shapes) != list(plan.band_shapes):
                raise ValueError("mask_layout='mosaic': the explainer's bands %s are not the evaluation plan's %s"
                                 % (xplan.band_shapes, plan.band_shapes))
            src, shape = wam_cell_source(plan, wam.frame, wam.method)
            cells = np.flatnonzero(src.reshape(-1) >= 0)
            ks = src.reshape(-1)[cells]
            assert np.unique(ks).size == ks.size and ks.max(initial=-1) < plan.coeff_numel, \
                "a coefficient is displayed by two cells"
            pos = np.full(plan.coeff_numel, shape[0] * shape[1], dtype=np.int32)
            pos[ks] = cells
            return torch.as_tensor(pos).to(dev), shape, int(plan.coeff_numel - ks.size)
        return device_table(("mosaic2d", plan, wam.mode, wam.frame, wam.method, dev), make)

    def _altered_inputs(self, img, masks):
        """masks [M, AH, AW] float32 device -> model inputs [M, 3, 224, 224] (or uint8 HWC numpy
        images when a host transform is set)."""
        dev = self._dev
        C, H, W = img.shape
        plan = get_plan(2, (H, W), self.J, self.wavelet, "symmetric", dev)  # pywt.wavedec2's default mode
        if self.mask_layout == "mosaic":
            pos, shape, _ = self._mosaic_layout(plan)
        else:
            pos, shape = self._layout(plan)
        if tuple(masks.shape[1:]) != tuple(shape):
            raise ValueError("operands could not be broadcast together with shapes (%d,%d) (%d,%d)"
                             % (shape + tuple(masks.shape[1:])))
        M = masks.shape[0]
        mask_len = shape[0] * shape[1]
        if self.mask_layout == "mosaic":  # the held slot: 1.0 in every mask
            masks = torch.cat([masks.reshape(M, -1), torch.ones((M, 1), dtype=torch.float32, device=dev)], 1)
            mask_len += 1
        coeffs = plan.wavedec(img.contiguous())
        masked = torch.empty(M * C * plan.coeff_numel, dtype=torch.float32, device=dev)
        check(lib.wam_coeff_masks(plan.handle, C, ptr(coeffs), ptr(pos), M, mask_len,
                                  ptr(masks.contiguous()), ptr(masked), stream_of(dev)))
        rec = plan.waverec(masked, M * C)[0]
        return self._model_inputs(plan, rec, M, C)

    def _ranked_inputs(self, imgs, wams, n_iter, deletion):
        """mask_layout='mosaic': imgs [G, C, H, W] on the device, wams [G, Hc, Wc] (host) -> the model
        inputs of all n_iter + 1 insertion (deletion) steps of every image, [G * (n_iter + 1), C, 224,
        224], image-major."""
        plan, rec = self._ranked_recs(imgs, wams, n_iter, deletion)
        return self._model_inputs(plan, rec, rec.shape[0] * rec.shape[1], rec.shape[2])

    def _ranked_recs(self, imgs, wams, n_iter, deletion):
        """-> (the evaluation plan, the masked reconstructions [G, n_iter + 1, C, rec_h, rec_w]): one
        wam_waverec2_ranked call, no mask stored."""
        dev = self._dev
        G, C, H, W = imgs.shape
        plan = get_plan(2, (H, W), self.J, self.wavelet, "symmetric", dev)
        pos, shape, _ = self._mosaic_layout(plan)
        wams = np.asarray(wams)
        if tuple(wams.shape[1:]) != tuple(shape):
            raise ValueError("operands could not be broadcast together with shapes (%d,%d) (%d,%d)"
                             % (shape + tuple(wams.shape[1:])))
        cells = shape[0] * shape[1]
        rank = descending_ranks(wams.reshape(G, cells), dev, self.tie_order)
        # the held slot: below every threshold under insertion, above every one under deletion
        held = torch.full((G, 1), np.iinfo(np.int32).max if deletion else -1, dtype=torch.int32, device=dev)
        rank = torch.cat([rank, held], 1).contiguous()
        coeffs = plan.wavedec(imgs.contiguous())
        rec = plan.waverec2_ranked(coeffs, G, C, rank, pos, n_iter, int(cells / n_iter), deletion,
                                   route=plan.ranked2_route() if self.ranked_route < 0 else self.ranked_route)
        return plan, rec

    def _model_inputs(self, plan, rec, M, C):
        """reconstructions of M images of C planes -> model inputs (the default transform on the device,
        a user transform on the host)."""
        dev = self._dev
        rh, rw = plan.rec_shape
        if self.transform is not None:
            return self._host_transform(rec.view(M, C, rh, rw))
        mean, std = norm_consts(C)
        if (rh, rw) == (224, 224):  # Resize((224, 224)) is the identity: one fused pass
            out = torch.empty((M, C, rh, rw), dtype=torch.float32, device=dev)
            check(lib.wam_quantize_normalize(M, C, rh * rw, ptr(rec), mean, std, ptr(out), stream_of(dev)))
            return out
        return self._resize_default(rec, M, C, rh, rw, mean, std)

    def _resize_default(self, rec, M, C, rh, rw, mean, std, size=(224, 224)):
        return resize_default(self._dev, rec, M, C, rh, rw, mean, std, size)[0]

    def _host_transform(self, rec):
        """The reference's PIL images (uint8 HWC -> PIL.Image.fromarray, src/evaluation_helpers.py
        reconstruct_images), then the user's transform (src/evaluators.py:631-633)."""
        from PIL import Image
        out = []
        for r in rec.double().cpu().numpy():
            d = np.moveaxis(r, 0, 2).astype(np.float32)
            u8 = (((d - d.min()) / (d.max() - d.min()).astype(np.float32)) * 255).astype(np.uint8)
            out.append(torch.as_tensor(np.asarray(self.transform(Image.fromarray(u8)))).float())
        return torch.stack(out).to(self._dev)

    def _rank_masks(self, wam, n_iter, deletion):
        hw = wam.shape[-2] * wam.shape[-1]
        rank = descending_ranks(np.reshape(wam, (1, -1)), self._dev, self.tie_order)
        masks = torch.empty((n_iter + 1, wam.shape[-2], wam.shape[-1]), dtype=torch.float32, device=self._dev)
        check(lib.wam_rank_masks(n_iter, int(hw / n_iter), hw, ptr(rank), int(bool(deletion)), ptr(masks),
                                 stream_of(self._dev)))
        return masks

    def _mask_hw(self, image_hw):
        """The shape the superpixel grid is zoomed to: the image's own, or the WAM canvas ('mosaic')."""
        if self.mask_layout != "mosaic":
            return tuple(int(v) for v in image_hw)
        plan = get_plan(2, tuple(int(v) for v in image_hw), self.J, self.wavelet, "symmetric", self._dev)
        return self._mosaic_layout(plan)[1]

    def _upsample(self, grid_masks, grid_size, hw):
        cell = cell_map(grid_size, hw, self._dev)
        g = torch.as_tensor(np.ascontiguousarray(grid_masks), dtype=torch.float32).to(self._dev)
        out = torch.empty((g.shape[0],) + tuple(hw), dtype=torch.float32, device=self._dev)
        check(lib.wam_upsample_masks(g.shape[0], grid_size * grid_size, ptr(g), hw[0] * hw[1], ptr(cell), ptr(out),
                                     stream_of(self._dev)))
        return out, cell

    def _evaluate_batched(self, images, label, batch_size):
        """evaluate() calls of the reference with its batch count int(ceil(len) / batch_size)."""
        n = images.shape[0]
        out = []
        for b in range(int(np.ceil(n) / batch_size)):
            s, e = b * batch_size, min(n, (b + 1) * batch_size)
            out.append(class_probs(self.model, images[s:e], label).astype(np.float32))
        return np.concatenate(out) if out else np.empty(0, dtype=np.float32)

    # -------------------------------------------------------------------- reference API
    def evaluate_auc(self, x, y, mode, n_iter=64):
        """src/evaluators.py:605-648: AUC of the class probability along the insertion
        (deletion) path of the WAM ranking; several images' masks per model forward."""
        if self.grad_wams is None:
            self.grad_wams = self.smooted_grad_wam(x, y)
        n_samples = self.grad_wams.shape[0]
        images = self._images(x)
        scores, predicted_probs = [], []
        per_call = max(1, self.eval_batch // (n_iter + 1))
        for s0 in range(0, n_samples, per_call):
            group = range(s0, min(n_samples, s0 + per_call))
            if self.mask_layout == "mosaic":
                inputs = self._ranked_inputs(torch.stack([images[s] for s in group]),
                                             np.stack([self.grad_wams[s] for s in group]), n_iter, mode == "deletion")
            else:
                inputs = torch.cat([self._altered_inputs(images[s], self._rank_masks(self.grad_wams[s], n_iter,
                                                                                    mode == "deletion"))
                                    for s in group])
            with torch.no_grad():
                preds = self.model(inputs).float().cpu().numpy()
            for p in class_curves(preds, n_iter + 1, [y[s] for s in group]):
                scores.append(compute_auc(p))
                predicted_probs.append(p)
        return scores, predicted_probs

    def insertion(self, x, y, n_iter=64):
        scores, predicted_probs = self.evaluate_auc(x, y, "insertion", n_iter=n_iter)
        self.insertion_curves = predicted_probs
        return scores

    def deletion(self, x, y, n_iter=64):
        scores, predicted_probs = self.evaluate_auc(x, y, "deletion", n_iter=n_iter)
        self.deletion_curves = predicted_probs
        return scores

    def mu_fidelity(self, x, y, grid_size=28, sample_size=128, subset_size=157):
        """src/evaluators.py:667-767."""
        if self.grad_wams is None:
            self.grad_wams = self.smooted_grad_wam(x, y)
        np.random.seed(self.random_seed)
        xd = torch.as_tensor(x).detach().to(self._dev, torch.float32)
        with torch.no_grad():
            base = softmax(self.model(xd).float().cpu().numpy())
        base_probs = [base[i, y[i]] for i in range(len(y))]
        images = self._images(x)
        H, W = self._mask_hw(xd.shape[2:])
        w, r = gaussian_weights(2)
        dev = self._dev
        mu = []
        for i in range(len(self.grad_wams)):
            g = torch.as_tensor(np.ascontiguousarray(self.grad_wams[i]), dtype=torch.float64).to(dev)
            wam = torch.empty_like(g)
            tmp = torch.empty_like(g)
            check(lib.wam_gaussian_filter2d(1, g.shape[0], g.shape[1], w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                            r, ptr(g), ptr(tmp), ptr(wam), stream_of(dev)))
            indices = generate_subsets(grid_size, subset_size, sample_size)
            bmask = self.compute_baseline_state(images[i], y[i], grid_size, self.batch_size, sample_size)
            masks = np.ones((sample_size, grid_size, grid_size))
            for j, index_set in enumerate(indices):
                cx, cy = zip(*index_set)
                masks[j, cx, cy] = bmask[cx, cy]
            up, cell = self._upsample(masks, grid_size, (H, W))
            altered = self._evaluate_batched(self._altered_inputs(images[i], up), y[i], self.batch_size)
            preds = base_probs[i] - altered
            sub = np.zeros((sample_size, grid_size, grid_size), dtype=np.float32)
            for j, index_set in enumerate(indices):
                cx, cy = zip(*index_set)
                sub[j, cx, cy] = 1
            mu.append(np.nanmean(spearmanr(preds, masked_sums(wam, sub, cell))))
        return mu

    def compute_baseline_state(self, image, label, grid_size, batch_size, sample_size):
        """src/evaluators.py:769-801: the uniform random superpixel mask whose reconstruction
        has the lowest class probability."""
        source_masks = np.random.uniform(size=(sample_size, grid_size, grid_size))
        up, _ = self._upsample(source_masks, grid_size, self._mask_hw(image.shape[1:]))
        ys = self._evaluate_batched(self._altered_inputs(image, up), label, batch_size)
        return source_masks[int(np.argmin(ys)), :, :]


# ====================================================================================== audio
def coeff_slot_map(length, levels, band_lens, n_masks=1):
    """The mask slot of every coefficient of a clip of `length` samples, as Eval1DWAM places its
    mask slices (src/evaluators.py:76-127): band i (coarse to fine, band_lens[i] = n_i coefficients)
    takes mask columns r[i] : max(r[i + 1], n_i) with r = [0, int(length / 2^J), ..., int(length / 2),
    length] -- offsets from the waveform length, not the bands' own running lengths -- clipped at the
    mask length sum(n_i). A slice n_i - 1 wide is padded on the right with one column (slot -1); any
    other width is numpy's broadcast ValueError of the reference's coeff * mask (n_masks only words
    the message). Returns int32 [sum(n_i)]."""
    total = int(sum(band_lens))
    r = [0] + [int(length / 2 ** j) for j in range(levels, -1, -1)]
    parts = []
    for i, n_i in enumerate(band_lens):
        start, end = r[i], min(max(r[i + 1], n_i), total)
        width = max(0, end - start)
        if width != n_i:
            width += 1  # np.pad(..., ((0, 0), (0, 1)))
            if width != n_i:
                raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,%d)"
                                 % (n_i, n_masks, width))
            parts.append(np.concatenate([np.arange(start, end), [-1]]))
        else:
            parts.append(np.arange(start, end))
    return np.concatenate(parts).astype(np.int32)


def coeff_identity_map(band_lens, grad_band_lens):
    """mask_layout='coeffs': the mask slot of every coefficient of the evaluation plan whose bands (A_J,
    D_J, ..., D_1) are band_lens long -- its own band-major per-item offset, pos[k] = k, so rank_len = K,
    no pad column and no held slot. grad_band_lens: the band lengths of the explainer's gradients, which
    must be the plan's. Returns int32 [sum(n_i)]."""
    if [int(n) for n in grad_band_lens] != [int(n) for n in band_lens]:
        raise ValueError("mask_layout='coeffs': the explainer's bands %s are not the evaluation plan's %s"
                         % ([int(n) for n in grad_band_lens], [int(n) for n in band_lens]))
    return np.arange(int(sum(band_lens)), dtype=np.int32)


def rank_thresholds(n_iter, rank_len):
    """(n_comp, [thr(0), ..., thr(n_iter)]) of a ranking with rank_len slots, as the rank-mask kernels
    apply them: n_comp = int(rank_len / n_iter), thr(0) = 0, thr(m) = min(m * n_comp, rank_len),
    thr(n_iter) = rank_len (insertion keeps the ranks below thr(m), deletion the others)."""
    n_comp = int(rank_len / n_iter)
    return n_comp, [0] + [min(m * n_comp, rank_len) for m in range(1, n_iter)] + [rank_len]


class Eval1DWAM(WaveletAttribution1D):
    """src/evaluators.py:39-306 -- insertion / deletion on the wavelet coefficients or on the mel
    spectrogram, faithfulness of spectra (Parekh et al.) and input fidelity (Paissan et al.) of an
    audio WAM, on the device. Same positional arguments, methods, return values and side attributes
    (``grad_wams`` computed once and cached, ``insertion_curves``, ``deletion_curves``).

    Per group of clips (``eval_batch`` model rows per forward, several clips' masks in one):

      wam_wavedec (ptwt's default mode 'reflect', not ``mode``) --ranks of |coefficient gradients| on
      the device--> wam_rank_mask_coeffs (all n_iter + 1 masked sets, band-major; the masks are never
      stored) --wam_waverec (one launch)--> wam_peak_normalize (wf / wf.max(), signed maximum)
      --mel front-end (k_mel_fwd where it applies, else the torch path)--> model (no grad)

    and for the mel target wam_rank_mask_rows on the clips' own dB mel spectrograms. Host work left:
    the softmax and AUC on [n_iter + 1, classes] logits, the ``tie_order='numpy'`` ranking.

    Kept from the reference: the mask slices are placed at offsets taken from the waveform length
    (coeff_slot_map; at 4004 samples they sit one slot off the gradients' own layout, at 4002 band 1
    takes a pad column that is 1 under insertion and 0 under deletion, every non-haar wavelet is a
    ValueError); the wavelet target ranks |g|, the mel target the signed gradient; the last mask is
    forced full. The all-zero mask reconstructs silence and 0 / 0 makes that row NaN, so every
    wavelet-target insertion / deletion score is NaN (``silent='nan'``, the default); k_mel_fwd's
    clamp would swallow a NaN waveform, so the rows wam_peak_normalize flags get NaN logits after
    the forward. ``silent='zero'`` leaves such a row silent and the scores finite. Ties: numpy's
    argsort is not stable; ``tie_order`` as in Eval2DWAM.

    ``mask_layout="coeffs"`` (an addition, opt-in; the default ``"reference"`` is the path above, bit for
    bit and call for call) scores every wavelet's maps on the wavelet target: each coefficient of the
    evaluation plan is ranked by its own gradient (the slot map is the identity on the band-major
    offset, rank_len = K = coeff_numel, no pad column; the explainer's band lengths must be the plan's,
    a ValueError otherwise), thr(m) = min(m * int(K / n_iter), K) with the last mask full. Per group of
    clips: one wam_wavedec, one wam_waverec1_ranked (all n_iter + 1 reconstructions and their signed
    maxima; ``ranked_route`` = -1 takes the plan's own route, 0 / 1 force one), one wam_peak_divide in
    place with the silent flags, then the same mel front-end and model. The silent end (insertion's
    first row, deletion's last) is handled by ``silent`` as above; the mel target has no layout."""

    def __init__(self, model, batch_size=128, wavelet="haar", J=3, method="smooth", mode="reflect", device=None,
                 approx_coeffs=False, n_mels=128, n_fft=1024, sample_rate=44100, n_samples=25, stdev_spread=0.001,
                 random_seed=42, *, tie_order="stable", eval_batch=520, silent="nan", mask_layout="reference",
                 **wam_kw):
        if mask_layout not in ("reference", "coeffs"):
            raise ValueError("mask_layout must be 'reference' or 'coeffs', got %r" % (mask_layout,))
        super().__init__(model, wavelet, J, method, mode, device, approx_coeffs, n_mels, n_fft, sample_rate, n_samples,
                         stdev_spread, random_seed)
        self.mask_layout = mask_layout
        self.ranked_route = -1  # 'coeffs': wam_waverec1_ranked's route, -1 = the plan's own (0 / 1 force one)
        self.grad_wams = None
        self.batch_size = batch_size
        self.gradwam = WaveletAttribution1D(model, wavelet=wavelet, J=J, method=method, mode=mode, device=device,
                                            approx_coeffs=approx_coeffs, n_mels=n_mels, n_fft=n_fft,
                                            sample_rate=sample_rate, n_samples=n_samples, stdev_spread=stdev_spread,
                                            random_seed=random_seed, **wam_kw)
        if silent not in ("nan", "zero"):
            raise ValueError("silent must be 'nan' or 'zero'")
        self.tie_order = check_tie_order(tie_order)
        self.eval_batch = eval_batch
        self.silent = silent
        self.insertion_curve = []   # the reference's constructor names
        self.deletion_curve = []
        self.insertion_curves = []
        self.deletion_curves = []

    # -------------------------------------------------------------------- device pipeline
    def _slot_map(self, plan, n_masks):
        return device_table(("slots1d", plan, self._dev), lambda: torch.as_tensor(
            coeff_slot_map(plan.shape[0], self.J, [s[0] for s in plan.band_shapes], n_masks)).to(self._dev))

    def _mel(self, wave):
        return db_melspec(wave, self.n_fft, self.sample_rate, self.n_mels)

    def auc_from_wavelet(self, gradients, waveform, sample, mode, n_iter):
        """src/evaluators.py:56-143 for the clips `sample` (an index or a sequence of indices) of
        `waveform` [N, W]: the dB mel spectrograms [len(sample) * (n_iter + 1), 1, T, n_mels] of the
        peak-normalised reconstructions of every masked coefficient set, on the device. The rows
        whose reconstruction is silent are left in ``self._silent_rows`` (bool, device)."""
        dev = self._dev
        samples = [sample] if np.isscalar(sample) else list(sample)
        wave = torch.as_tensor(waveform).detach().to(dev, torch.float32)
        # the reference's call hands over the clip itself (x[sample]); a batch is indexed here
        wave = (wave[None] if wave.dim() == 1 else wave[samples]).contiguous()
        sets, M = len(samples), n_iter + 1
        plan = get_plan(1, (wave.shape[-1],), self.J, self.wavelet, "reflect", dev)  # ptwt.wavedec's default mode
        if self.mask_layout == "coeffs":
            return self._auc_from_coeffs(plan, gradients, wave, samples, mode, n_iter)
        pos = self._slot_map(plan, M)
        K = plan.coeff_numel
        g = np.stack([np.concatenate([np.asarray(b)[s] for b in gradients]) for s in samples])
        if g.shape[1] != K:
            raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,%d)" % (K, M, g.shape[1]))
        rank = descending_ranks(np.abs(g), dev, self.tie_order)
        coeffs = plan.wavedec(wave)
        masked = torch.empty(sets * M * K, dtype=torch.float32, device=dev)
        check(lib.wam_rank_mask_coeffs(plan.handle, sets, ptr(coeffs), ptr(rank), K, ptr(pos), n_iter, int(K / n_iter),
                                       int(mode == "deletion"), ptr(masked), stream_of(dev)))
        rec = plan.waverec(masked, sets * M)[0].view(sets * M, -1)
        flags = torch.empty(sets * M, dtype=torch.int32, device=dev)
        check(lib.wam_peak_normalize(sets * M, rec.shape[1], ptr(rec), ptr(rec), ptr(flags),
                                     int(self.silent == "zero"), stream_of(dev)))
        self._silent_rows = flags.bool()
        return self._mel(rec)

    def _auc_from_coeffs(self, plan, gradients, wave, samples, mode, n_iter):
        """auc_from_wavelet under mask_layout='coeffs': wave [sets, W] on the device."""
        dev = self._dev
        sets, M, K = len(samples), n_iter + 1, plan.coeff_numel
        band_lens = [s[0] for s in plan.band_shapes]
        pos_host = coeff_identity_map(band_lens, [np.asarray(b).shape[1] for b in gradients])
        pos = device_table(("coeffs1d", plan, dev), lambda: torch.as_tensor(pos_host).to(dev))
        g = np.stack([np.concatenate([np.asarray(b)[s] for b in gradients]) for s in samples])
        rank = descending_ranks(np.abs(g), dev, self.tie_order)
        coeffs = plan.wavedec(wave)
        rec, row_max = plan.waverec1_ranked(coeffs, sets, rank, pos, n_iter, rank_thresholds(n_iter, K)[0],
                                            mode == "deletion", route=self.ranked_route)
        rec, flags = peak_divide(rec.view(sets * M, -1), row_max, zero_silent=self.silent == "zero")
        self._silent_rows = flags.bool()
        return self._mel(rec)

    def auc_from_melspec(self, melspec, source_melspec, mode, n_iter):
        """src/evaluators.py:145-176 for one clip ([T, n_mels] gradients and dB mel spectrogram) or a
        batch of clips ([sets, T, n_mels]): [sets * (n_iter + 1), 1, T, n_mels] on the device."""
        self._silent_rows = None
        return rank_mask_rows(melspec, source_melspec, n_iter, mode == "deletion", self._dev, self.tie_order)

    # -------------------------------------------------------------------- reference API
    def evaluate_auc(self, x, y, mode, target, n_iter=64, argmax=False):
        """src/evaluators.py:178-235."""
        if isinstance(x, list):
            x = _peak_normalise_1d(x)
        if self.grad_wams is None:
            self.grad_wams = self.gradwam(x, y)
        dev = self._dev
        xd = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
        melspecs, gradients = self.grad_wams
        n_sounds = xd.shape[0]
        M = n_iter + 1
        scores, predicted_probs, raw_preds = [], [], []
        per_call = max(1, self.eval_batch // M)
        with torch.no_grad():
            source = self._mel(xd) if target == "melspec" else None
            for s0 in range(0, n_sounds, per_call):
                group = list(range(s0, min(n_sounds, s0 + per_call)))
                if target == "melspec":
                    inputs = self.auc_from_melspec(np.asarray(melspecs)[group], source[group], mode, n_iter)
                elif target == "wavelet":
                    inputs = self.auc_from_wavelet(gradients, xd, group, mode, n_iter)
                else:
                    raise ValueError("target must be 'wavelet' or 'melspec', got %r" % (target,))
                logits = self.model(inputs).float()
                if self._silent_rows is not None and self.silent == "nan":
                    logits[self._silent_rows] = float("nan")
                preds = logits.cpu().numpy()
                raw_preds.extend(preds.reshape(len(group), M, -1))
                for prob in class_curves(preds, M, [y[s] for s in group]):
                    scores.append(compute_auc(prob))
                    predicted_probs.append(prob)
        if argmax:
            return raw_preds
        return scores, predicted_probs

    def insertion(self, x, y, target, n_iter):
        scores, predicted_probs = self.evaluate_auc(x, y, "insertion", target, n_iter)
        self.insertion_curves = predicted_probs
        return scores

    def deletion(self, x, y, target, n_iter):
        scores, predicted_probs = self.evaluate_auc(x, y, "deletion", target, n_iter)
        self.deletion_curves = predicted_probs
        return scores

    def faithfulness_of_spectra(self, x, y, target):
        """src/evaluators.py:247-277: the drop of the class probability when the more important half
        of the components is deleted (deletion with n_iter = 2, p[0] - p[1])."""
        _, predicted_probs = self.evaluate_auc(x, y, "deletion", target, 2)
        predicted_probs = np.array(predicted_probs)
        return (predicted_probs[:, 0] - predicted_probs[:, 1]).tolist()

    def input_fidelity(self, x, y, target):
        """src/evaluators.py:279-306: arg-max classes with the more important half and with all of the
        components inserted (insertion with n_iter = 2, rows 1 and 2)."""
        preds = np.array(self.evaluate_auc(x, y, "insertion", target, 2, argmax=True))
        return np.argmax(preds[:, 1:, :], axis=2).tolist()
