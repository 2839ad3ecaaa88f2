"""Necessary components and scale isolation of a 2D WAM on MI355X.

Drop-in for the reference's ``WAMAnalyzer2D`` (``src/analyzers.py:16-203``) and the helpers it calls
(``src/analyzers_helpers.py:6-134``): same class, constructor order and defaults, methods, return
values and side attributes (``grad_wams`` computed once and cached, ``insertion_quantile``,
``deletion_quantile``, ``smooted_grad_wam``). Per image and per quantile the reference runs three
pywt.wavedec2, a boolean mask on pywt's coeffs_to_array array, three pywt.waverec2, a uint8 round trip
through PIL and the transform, all on the CPU. Here, per group of images (``eval_batch`` model inputs
per forward):

  show()-normalised planes --wam_wavedec (pywt's default mode 'symmetric', once on all N * 3 planes)-->
  coefficients --wam_threshold_mask_coeffs (every image x threshold x channel plane, band-major; the
  masks are never stored)--> wam_waverec (one launch) --wam_quantize_normalize_ex (the analyzer's own
  quantisation, bytes for the returned PIL images + ToTensor + ImageNet Normalize)--> model (no grad)

The thresholds are numpy's linear quantiles of each map (one torch.sort per map, the two order
statistics gathered, numpy's _lerp in float64) or, for isolate_scales, ``min(0, region min) + EPS``
per level entry. Host work left: the softmax and arg-max on [len(qs), classes] logits, the three PIL
images returned per input and ``mask * grad_wam`` of the chosen quantile.

Kept from the reference (pinned by tests/golden/analyzer_goldens.npz, made by the reference's own
helpers with PyWavelets 1.1.1):
  * the mask multiplies pywt's coeffs_to_array array (cH bottom-left, cV top-right -- transposed
    relative to the WAM mosaic), so the map's shape must equal that array's: haar with S % 2^J == 0;
    anything else is numpy's broadcast ValueError, as is a non-square input;
  * the quantisation is ``((x - mn) / mx - mn) * 255`` -- operator precedence makes it
    ((x - mn) / mx - mn) * 255, not a min-max -- followed by ``.astype(np.uint8)``, which wraps: most
    grey levels fall outside [0, 256) and only their low 8 bits survive. That wrapped image is what
    the reference's model sees, so it is the default here (``normalize='reference'``);
    ``normalize='minmax'`` is Eval2DWAM's min-max instead;
  * the constructor hands ``method`` to the inner explainer but not ``n_samples`` / ``stdev_spread`` /
    ``random_seed``, which are only stored as attributes; the outer class is built with
    method='smooth' whatever the caller passes;
  * ``correct_index`` is the last correct prediction under 'deletion' and the first under
    'insertion'; without a correct prediction the tuple is ((None, None, None), None, grad_wam,
    (None, nan)) and no quantile is appended.
Not kept: generate_disentangled_images' stray print; an unknown ``mode`` string is a ValueError (the
reference runs into an unbound name).
"""
import ctypes

import numpy as np
import torch

from ._lib import c_vp, check, lib, ptr, stream_of
from .evalcore import array_layout, device_table, norm_consts, resize_default, show_images, softmax
from .plan import get_plan
from .wam_2D import WaveletAttribution2D

RULES = {"minmax": 0, "reference": 1}


# ------------------------------------------------------------------------------ host geometry
def compute_levelized_masks(grad_wam, J):
    """src/analyzers_helpers.py:6-33: [J + 1, S, S] float64, entry j < J (finest first) = grad_wam on
    the three detail blocks of level j, entry J = grad_wam on the approximation block, 0 elsewhere."""
    size = grad_wam.shape[0]
    out = np.zeros((J + 1, size, size))
    for j in range(J):
        s, e = int(size / 2 ** (j + 1)), int(size / 2 ** j)
        out[j, s:e, s:e] = grad_wam[s:e, s:e]
        out[j, s:e, :s] += grad_wam[s:e, :s]
        out[j, :s, s:e] += grad_wam[:s, s:e]
    a = int(size / 2 ** J)
    out[J, :a, :a] = grad_wam[:a, :a]
    return out


def level_edges(size, J):
    """int(size / 2^j), j = 0 .. J: the `edges` table of wam_threshold_mask_coeffs' level mode."""
    return [int(size / 2 ** j) for j in range(J + 1)]


def _level_entry_map(size, J, dev):
    """[size * size] int64 on `dev`: the level entry whose region holds each position (-1: none)."""
    def make():
        e = level_edges(size, J)
        m = np.maximum(np.arange(size)[:, None], np.arange(size)[None, :])
        entry = np.full((size, size), -1, dtype=np.int64)
        for j in range(J):
            entry[(m >= e[j + 1]) & (m < e[j])] = j
        entry[m < e[J]] = J
        return torch.as_tensor(entry.reshape(-1)).to(dev)
    return device_table(("levels2d", size, J, dev), make)


# ------------------------------------------------------------------------------ thresholds
def quantile_thresholds(maps, qs):
    """np.quantile(map, q) (method 'linear') of every row of maps [N, L] float64 (device) for every q:
    [N, len(qs)] float64 on the device. The virtual index is (L - 1) * q in float64, the two order
    statistics a <= b around it come from one sort per map, and the interpolation is numpy's _lerp:
    a + (b - a) * g, replaced by b - (b - a) * (1 - g) where g >= 0.5."""
    L = maps.shape[1]
    q = np.asarray(qs, dtype=np.float64).reshape(-1)
    if q.size and (q.min() < 0 or q.max() > 1):
        raise ValueError("Quantiles must be in the range [0, 1]")
    vi = (L - 1) * q
    lo = np.floor(vi)
    g = torch.as_tensor(vi - lo).to(maps.device)
    lo = np.clip(lo.astype(np.int64), 0, L - 1)
    hi = np.clip(lo + 1, 0, L - 1)
    srt = torch.sort(maps, dim=1).values
    a = srt[:, torch.as_tensor(lo).to(maps.device)]
    b = srt[:, torch.as_tensor(hi).to(maps.device)]
    d = b - a
    return torch.where(g >= 0.5, b - d * (1 - g), a + d * g).contiguous()


def level_thresholds(maps, size, J, eps):
    """filtered_masks[l].min() + EPS of compute_levelized_masks for every map [N, size * size] float64
    (device): the minimum runs over the whole array, zeros outside the entry's region included, so it is
    min(0, region min). [N, J + 1] float64 on the device."""
    entry = _level_entry_map(size, J, maps.device)
    cols = []
    for l in range(J + 1):
        inside = maps.masked_fill(entry != l, float("inf")).amin(dim=1)
        cols.append(torch.minimum(inside, torch.zeros_like(inside)) + float(eps))
    return torch.stack(cols, dim=1).contiguous()


# ------------------------------------------------------------------------------ device pipeline
def _square_plan(planes, wam_shape, J, wavelet, dev):
    H, W = planes.shape[-2:]
    plan = get_plan(2, (H, W), J, wavelet, "symmetric", dev)  # pywt.wavedec2's default mode
    pos, shape = array_layout(plan, dev)
    if tuple(shape) != tuple(wam_shape) or shape[0] != shape[1]:
        raise ValueError("operands could not be broadcast together with shapes (%d,%d) (%d,%d)"
                         % (tuple(shape) + tuple(wam_shape)))
    return plan, pos, shape[0]


def match_counts(n_images, grad_wams, reference_zip=False):
    """The number of images to process, checked on the host before any launch: the kernel reads map and
    threshold row n for image n, so the maps must cover the images. Fewer maps than images is the
    reference's IndexError (its loop indexes grad_wams by the image number); isolate_scales zips the two
    instead (reference_zip) and stops at the shorter one. Surplus maps are left unused, as there."""
    n_maps = int(np.shape(grad_wams)[0])
    if reference_zip:
        return min(n_images, n_maps)
    if n_maps < n_images:
        raise IndexError("index %d is out of bounds for axis 0 with size %d (grad_wams holds %d maps for %d images)"
                         % (n_maps, n_maps, n_maps, n_images))
    return n_images


def plane_coeffs(plan, coeffs, total, p0, p1):
    """The band-major coefficients of planes p0 .. p1 - 1 out of a band-major buffer over `total` planes, as
    a band-major buffer of their own (the input itself when that is all of them)."""
    if p0 == 0 and p1 == total:
        return coeffs
    return torch.cat([v[p0:p1].reshape(-1) for v in plan.split(coeffs, total)])


def masked_reconstructions(plan, pos, size, planes, maps, thr, q0=0, n_thr=None, level=False, strict=False, edges=None,
                           coeffs=None):
    """planes [N, C, H, W] float32, maps [N, size * size] float64, thr [N, Q] float64 (all on the
    device) -> the reconstructions [N, n_thr, C, H', W'] of the coefficients masked by thresholds
    q0 .. q0 + n_thr - 1 of every image: wam_wavedec (skipped when the planes' band-major `coeffs` are
    given), wam_threshold_mask_coeffs, wam_waverec. Every buffer length the kernel relies on is checked here."""
    dev = planes.device
    N, C = planes.shape[:2]
    n_thr = thr.shape[1] - q0 if n_thr is None else n_thr
    K = plan.coeff_numel
    if tuple(maps.shape) != (N, size * size) or thr.dim() != 2 or thr.shape[0] != N:
        raise ValueError("maps %s and thresholds %s do not match %d images of %d x %d positions"
                         % (tuple(maps.shape), tuple(thr.shape), N, size, size))
    if q0 < 0 or n_thr < 1 or q0 + n_thr > thr.shape[1]:
        raise ValueError("thresholds %d .. %d are outside the %d of a row" % (q0, q0 + n_thr - 1, thr.shape[1]))
    if pos.numel() != K or (level and (edges is None or len(edges) != n_thr)):
        raise ValueError("position table or level edges do not match the plan")
    for t, dt in ((maps, torch.float64), (thr, torch.float64), (pos, torch.int32)):
        if t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError("maps / thresholds (float64) and positions (int32) must be contiguous on %s" % (dev,))
    if coeffs is None:
        coeffs = plan.wavedec(planes.contiguous())
    elif coeffs.numel() != N * C * K or coeffs.dtype != torch.float32 or coeffs.device != dev:
        raise ValueError("coefficients do not match %d planes of the plan" % (N * C))
    masked = torch.empty(N * n_thr * C * K, dtype=torch.float32, device=dev)
    ed = None if edges is None else (ctypes.c_int32 * len(edges))(*edges)
    check(lib.wam_threshold_mask_coeffs(plan.handle, N, C, ptr(coeffs.contiguous()), ptr(pos), size, ptr(maps), n_thr,
                                        c_vp(thr.data_ptr() + 8 * q0), thr.shape[1], int(bool(level)), ed,
                                        int(bool(strict)), ptr(masked), stream_of(dev)))
    rec = plan.waverec(masked, N * n_thr * C)[0]
    return rec.view((N, n_thr, C) + tuple(plan.rec_shape))


def _device(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _maps_on(grad_wams, dev):
    g = torch.as_tensor(np.ascontiguousarray(grad_wams), dtype=torch.float64).to(dev)
    return g.reshape(g.shape[0], -1).contiguous()


def generate_partial_image(img, grad_wam, q, J, wavelet="haar"):
    """src/analyzers_helpers.py:35-81 on the device: img [S, S, 3] (show()'s HWC array), grad_wam
    [S, S] -> (the image rebuilt from the coefficients whose map value is >= np.quantile(grad_wam, q),
    [S, S, 3] float32; mask * grad_wam, [S, S])."""
    dev = _device()
    grad_wam = np.asarray(grad_wam)
    planes = torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(img, dtype=np.float32), 2, 0))).to(dev)[None]
    plan, pos, size = _square_plan(planes, grad_wam.shape, J, wavelet, dev)
    maps = _maps_on(grad_wam[None], dev)
    thr = quantile_thresholds(maps, [q])
    rec = masked_reconstructions(plan, pos, size, planes, maps, thr)
    t = float(thr[0, 0])
    return rec[0, 0].permute(1, 2, 0).contiguous().cpu().numpy(), (grad_wam >= t) * grad_wam


def _disentangled(planes, grad_wams, J, eps, wavelet, dev):
    """[N, J + 1, S, S, 3] float64 (device): np.clip(rec, 0, 255) of every level entry's reconstruction."""
    plan, pos, size = _square_plan(planes, np.shape(grad_wams)[1:], J, wavelet, dev)
    maps = _maps_on(grad_wams, dev)
    thr = level_thresholds(maps, size, J, eps)
    rec = masked_reconstructions(plan, pos, size, planes, maps, thr, level=True, strict=True,
                                 edges=level_edges(size, J))
    return rec.clamp(0, 255).permute(0, 1, 3, 4, 2).double()


def generate_disentangled_images(grad_wam, image, J, EPS=0.1, wavelet="haar"):
    """src/analyzers_helpers.py:83-134 on the device: (partial_images [J + 1, S, S, 3] float64, the
    image rebuilt from each level's coefficients whose map value exceeds the entry's minimum + EPS,
    finest level first, the approximation last, clipped to [0, 255]; filtered_masks [J + 1, S, S])."""
    dev = _device()
    grad_wam = np.asarray(grad_wam)
    planes = torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(image, dtype=np.float32), 2, 0))).to(dev)[None]
    out = _disentangled(planes, grad_wam[None], J, EPS, wavelet, dev)
    return out[0].cpu().numpy(), compute_levelized_masks(grad_wam, J)


class WAMAnalyzer2D(WaveletAttribution2D):
    """src/analyzers.py:16-203 -- isolate_scales: the image split into what each scale's important
    coefficients rebuild; isolate_necessary_components: the model evaluated on images rebuilt from ever
    more (insertion) or ever fewer (deletion) of the most important coefficients."""

    def __init__(self, model, wavelet="haar", J=3, device=None, mode="reflect", approx_coeffs=False, method="smooth",
                 n_samples=25, stdev_spread=0.25, random_seed=42, *, eval_batch=520, normalize="reference", **wam_kw):
        super().__init__(model, wavelet=wavelet, J=J, device=device, method="smooth", mode=mode,
                         approx_coeffs=approx_coeffs)
        self.n_samples = n_samples
        self.stdev_spread = stdev_spread
        self.random_seed = random_seed
        # as the reference: the caller's method, but the inner explainer's own sampling defaults
        self.smooted_grad_wam = WaveletAttribution2D(model, wavelet=wavelet, J=J, method=method, mode=mode,
                                                     approx_coeffs=approx_coeffs, device=device, **wam_kw)
        if normalize not in RULES:
            raise ValueError("normalize must be 'reference' or 'minmax'")
        if int(eval_batch) < 1:
            raise ValueError("eval_batch must be at least 1")
        self.normalize = normalize
        self.eval_batch = int(eval_batch)
        self.grad_wams = None
        self.insertion_quantile = []
        self.deletion_quantile = []

    # -------------------------------------------------------------------- device pipeline
    def _inputs(self, rec, transform):
        """rec [M, C, H, W] -> (model inputs, the quantised bytes [M, C, H * W] on the device)."""
        dev = self._dev
        M, C, rh, rw = rec.shape
        rule = RULES[self.normalize]
        rec = rec.contiguous()
        if transform is not None:
            u8 = torch.empty((M, C, rh * rw), dtype=torch.uint8, device=dev)
            check(lib.wam_quantize_normalize_ex(M, C, rh * rw, ptr(rec), rule, None, None, ptr(u8), None,
                                                stream_of(dev)))
            host = u8.view(M, C, rh, rw).permute(0, 2, 3, 1).contiguous().cpu().numpy()
            return torch.stack([transform(self._pil(h)) for h in host]).to(dev), u8
        mean, std = norm_consts(C)
        if (rh, rw) == (224, 224):  # Resize((224, 224)) is the identity: one fused pass
            u8 = torch.empty((M, C, rh * rw), dtype=torch.uint8, device=dev)
            out = torch.empty((M, C, rh, rw), dtype=torch.float32, device=dev)
            check(lib.wam_quantize_normalize_ex(M, C, rh * rw, ptr(rec), rule, mean, std, ptr(u8), ptr(out),
                                                stream_of(dev)))
            return out, u8
        return resize_default(dev, rec, M, C, rh, rw, mean, std, rule=rule)

    @staticmethod
    def _pil(hwc):
        from PIL import Image
        return Image.fromarray(hwc)

    def _image_of(self, u8, hw):
        """One item's planar bytes [C, H * W] (device) -> the reference's PIL image."""
        return self._pil(u8.view(u8.shape[0], hw[0], hw[1]).permute(1, 2, 0).contiguous().cpu().numpy())

    # -------------------------------------------------------------------- reference API
    def isolate_scales(self, x, y, EPS=0.1):
        """src/analyzers.py:73-92: per image (partial_images [J + 1, S, S, 3] float64, filtered_masks
        [J + 1, S, S] float64), all images and levels in one pass."""
        if self.grad_wams is None:
            self.grad_wams = self.smooted_grad_wam(x, y)
        n = match_counts(len(x), self.grad_wams, reference_zip=True)   # host check, before any launch
        if n == 0:
            return []
        planes = torch.stack(show_images(x[:n], self._dev))
        out = _disentangled(planes, np.asarray(self.grad_wams)[:n], self.J, EPS, self.wavelet, self._dev).cpu().numpy()
        return [(out[i], compute_levelized_masks(np.asarray(self.grad_wams[i]), self.J)) for i in range(n)]

    def isolate_necessary_components(self, x, y, qs, transform=None, mode=None):
        """src/analyzers.py:94-203: per image ((first, chosen, last PIL image), mask * grad_wam of the
        chosen quantile, grad_wam, (probs [len(qs), classes], correct_index))."""
        if mode is None:
            print("Input a mode, either 'insertion' or 'deletion'")
            raise ValueError
        if mode not in ("insertion", "deletion"):
            raise ValueError("mode must be 'insertion' or 'deletion', got %r" % (mode,))
        if mode == "deletion":
            assert qs[0] <= qs[1]
        if mode == "insertion":
            assert qs[0] >= qs[1]
        if self.grad_wams is None:
            self.grad_wams = self.smooted_grad_wam(x, y)
        N, Q = match_counts(len(x), self.grad_wams), len(qs)   # host check, before any launch
        dev = self._dev
        planes = torch.stack(show_images(x, dev))
        plan, pos, size = _square_plan(planes, np.shape(self.grad_wams)[1:], self.J, self.wavelet, dev)
        maps = _maps_on(np.asarray(self.grad_wams)[:N], dev)
        coeffs = plan.wavedec(planes)   # once, all N * 3 planes
        C = planes.shape[1]
        thr = quantile_thresholds(maps, qs)
        thr_host = thr.cpu().numpy()
        hw = tuple(plan.rec_shape)
        q_step = min(Q, self.eval_batch)
        per_call = max(1, self.eval_batch // Q)
        outs = []
        for n0 in range(0, N, per_call):
            n1 = min(N, n0 + per_call)
            preds, bytes_ = [], []
            group = plane_coeffs(plan, coeffs, N * C, n0 * C, n1 * C)
            for q0 in range(0, Q, q_step):
                nq = min(q_step, Q - q0)
                rec = masked_reconstructions(plan, pos, size, planes[n0:n1], maps[n0:n1], thr[n0:n1], q0, nq,
                                             coeffs=group)
                inputs, u8 = self._inputs(rec.view((-1,) + tuple(rec.shape[2:])), transform)
                with torch.no_grad():
                    p = self.model(inputs).float().cpu().numpy()
                preds.append(p.reshape(n1 - n0, nq, -1))
                bytes_.append(u8.view(n1 - n0, nq, u8.shape[1], -1))
            preds = np.concatenate(preds, axis=1)
            u8 = bytes_[0] if len(bytes_) == 1 else torch.cat(bytes_, dim=1)
            for k, index in enumerate(range(n0, n1)):
                grad_wam = self.grad_wams[index]
                probs = softmax(preds[k])
                hits = np.where(np.argmax(preds[k], axis=1) == y[index])[0]
                if not len(hits):
                    outs.append(((None, None, None), None, grad_wam, (None, np.nan)))
                    continue
                if mode == "deletion":
                    correct_index = hits[-1]
                    self.deletion_quantile.append(qs[correct_index])
                else:
                    correct_index = hits[0]
                    self.insertion_quantile.append(qs[correct_index])
                images = tuple(self._image_of(u8[k, i], hw) for i in (0, int(correct_index), Q - 1))
                mask = (np.asarray(grad_wam) >= thr_host[index, correct_index]) * np.asarray(grad_wam)
                outs.append((images, mask, grad_wam, (probs, correct_index)))
        return outs
