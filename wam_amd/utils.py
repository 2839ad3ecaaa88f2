"""Drop-in for the reference's top-level ``utils.py`` and the agreement measures of its
``compare_iou_models.ipynb``, with the map statistics on the device.

    from wam_amd.utils import *          # was: from utils import ...

What a WAM map is used for once it exists: how much attribution sits on each scale
(get_gradients_attribution_on_levels, level_shares), how much the detail levels disagree pixel by
pixel (get_mean_pixelwise_variance), which images disagree most (rank_images) and how well the
top-p % regions of several explainers coincide (mean_pairwise_iou, get_iou_between_wavelets). The
reference copies every float64 map to the host and loops scipy.ndimage.zoom, np.var, np.argsort and
boolean reductions per image; here the maps stay where the explainer left them (BaseWAM2D.map_device)
and two entry points of libwam_hip.so do the work (wam_level_stats, wam_mask_iou;
wam_amd/csrc/scalestats.hip). Names, positional arguments and return types are the reference's.

The map-taking functions accept a numpy array ([H, H] or [N, H, H], uploaded once) or a float64
device tensor. There is no host fallback: without a HIP device they raise.
"""
import ctypes

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_of
from .plan import reproject_scales

__all__ = ["get_explanations_for_image", "get_diagonal", "get_mean_pixelwise_variance", "rank_images",
           "get_gradients_attribution_on_levels", "get_multiple_grad_attr", "get_mean_across_images", "level_shares",
           "get_highest_percentage", "iou", "get_grad_reprojection", "mean_pairwise_iou",
           "get_iou_between_wavelets"]

_WAM_ERR_SHAPE = 2
_WAM_ERR_UNSUPPORTED = 3


def _iou_limits():
    """(maps, percentages) one wam_mask_iou launch takes, asked of the library; above them the call
    answers WAM_ERR_UNSUPPORTED and _mask_counts runs pair and percentage chunks."""
    m, q = ctypes.c_int(0), ctypes.c_int(0)
    lib.wam_mask_iou_limits(ctypes.byref(m), ctypes.byref(q))
    return m.value, q.value


# ---------------------------------------------------------------------------------------- inputs

def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("wam_amd.utils: the map statistics run on the GPU only (no HIP device found)")
    return torch.device("cuda", torch.cuda.current_device())


def _on_device(x):
    """numpy array, list of arrays or of tensors, or tensor -> float64 device tensor (one upload)."""
    if isinstance(x, torch.Tensor):
        g = x.detach()
        return (g if g.device.type == "cuda" else g.to(_device())).to(torch.float64)
    if isinstance(x, (list, tuple)) and len(x) and isinstance(x[0], torch.Tensor):
        return torch.stack([t.detach().to(_device(), torch.float64) for t in x])
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(_device())


def _maps_dev(grad_wam):
    """[H, W] or [N, H, W] -> float64 device [N, H, W], contiguous."""
    g = _on_device(grad_wam)
    if g.dim() == 2:
        g = g[None]
    if g.dim() != 3:
        raise ValueError("expected a [H, H] map or [N, H, H] maps, got shape %s" % (tuple(g.shape),))
    assert g.shape[1] == g.shape[2], "grad_wam must be square"
    return g.contiguous()


# ----------------------------------------------------------------------------------- level stats

def _detail_sides(H, J):
    return [H // (2 ** j) - H // (2 ** (j + 1)) for j in range(J)]


def _zoom_lengths(H, J, size):
    """(T, scipy.ndimage.zoom's output length per detail level) of get_mean_pixelwise_variance."""
    sizes = _detail_sides(H, J)
    if size == "maximal":
        target = max(sizes)
    elif size == "minimal":
        target = min(sizes)
    else:
        raise ValueError("size must be 'maximal' or 'minimal'")
    lens = []
    for n in sizes:
        scale = target / n  # ZeroDivisionError on an empty level, as in the reference
        lens.append(int(round(n * scale)))
    if any(m < target for m in lens):
        raise ValueError("all input arrays must have the same shape")  # the reference's np.stack
    return target, lens


def _level_stats(maps, J, size=None, want_abs=False, want_map=False, want_mean=False):
    """One wam_level_stats launch over maps [N, H, H] -> (abs_sums, var_map, mean_var), device
    tensors or None."""
    N, H = int(maps.shape[0]), int(maps.shape[1])
    J = int(J)
    target, lens = (0, None)
    if want_map or want_mean:
        target, lens = _zoom_lengths(H, J, size)
    dev = maps.device
    abs_sums = torch.empty((N, J + 1), dtype=torch.float64, device=dev) if want_abs else None
    var_map = torch.empty((N, target, target), dtype=torch.float64, device=dev) if want_map else None
    mean_var = torch.empty((N,), dtype=torch.float64, device=dev) if want_mean else None
    if N == 0:
        return abs_sums, var_map, mean_var
    ws_bytes = int(lib.wam_level_stats_ws_bytes(N, H, J, target))
    if ws_bytes < 0:
        raise ValueError("wam_level_stats: unsupported size %d / levels %d" % (H, J))
    ws = torch.empty((max(ws_bytes // 8, 1),), dtype=torch.float64, device=dev)
    c_lens = (ctypes.c_int32 * len(lens))(*lens) if lens else None
    with torch.cuda.device(dev):
        rc = lib.wam_level_stats(N, H, J, ptr(maps), target, c_lens, ptr(abs_sums), ptr(var_map), ptr(mean_var),
                                 ptr(ws), ws_bytes, stream_of(dev))
    if rc == _WAM_ERR_SHAPE:
        raise ValueError("all input arrays must have the same shape")
    check(rc)
    return abs_sums, var_map, mean_var


def get_diagonal(grad_wam, J):
    """The diagonal blocks of a WAM map, as views: level_0 ... level_{J-1} (details, finest first),
    then approx (the coarsest scale)."""
    H, W = grad_wam.shape
    assert H == W, "grad_wam must be square"
    diagonals = {}
    for j in range(J):
        start, end = H // (2 ** (j + 1)), H // (2 ** j)
        diagonals["level_%d" % j] = grad_wam[start:end, start:end]
    a = H // (2 ** J)
    diagonals["approx"] = grad_wam[:a, :a]
    return diagonals


def get_mean_pixelwise_variance(grad_wam, J, size="maximal"):
    """Pixel-wise variance between the detail levels, each resized (scipy.ndimage.zoom, order 1) to
    the largest ("maximal") or smallest ("minimal") level -> (mean_variance: float, variance_map:
    ndarray [T, T]). One launch."""
    if len(grad_wam.shape) != 2:
        raise ValueError("grad_wam must be one [H, H] map, got shape %s" % (tuple(grad_wam.shape),))
    assert grad_wam.shape[0] == grad_wam.shape[1], "grad_wam must be square"
    _zoom_lengths(int(grad_wam.shape[0]), int(J), size)  # the reference's errors, before anything is uploaded
    maps = _maps_dev(grad_wam)
    _, var_map, mean_var = _level_stats(maps, J, size, want_map=True, want_mean=True)
    return float(mean_var.cpu()[0]), var_map[0].cpu().numpy()


def rank_images(explanations, J, size="maximal"):
    """Images ranked by cross-level pixel-wise variance, descending (ties keep image order):
    [{"image_index": int, "mean_pixelwise_variance": float}, ...]. One launch for all images, one
    transfer of N doubles; no variance map is stored."""
    if len(explanations) == 0:
        return []
    maps = _maps_dev(explanations)
    _, _, mean_var = _level_stats(maps, J, size, want_mean=True)
    mv = mean_var.cpu().numpy()
    ranking = [{"image_index": idx, "mean_pixelwise_variance": float(v)} for idx, v in enumerate(mv)]
    ranking.sort(key=lambda x: x["mean_pixelwise_variance"], reverse=True)
    return ranking


def _shares(abs_sums):
    out = []
    for row in abs_sums:
        row = np.array(row)
        row /= np.sum(row)
        out.append(row)
    return out


def level_shares(maps, J):
    """float64 [N, J + 1]: each map's sum |v| over level_0 ... level_{J-1}, approx, divided by their
    total -- what get_gradients_attribution_on_levels returns, for maps already at hand."""
    if len(maps) == 0:
        return np.empty((0, int(J) + 1), dtype=np.float64)
    abs_sums, _, _ = _level_stats(_maps_dev(maps), J, want_abs=True)
    return np.array(_shares(abs_sums.cpu().numpy())).reshape(abs_sums.shape[0], int(J) + 1)


def get_explanations_for_image(image, model, explainer, transform, device, J):
    """The explainer's map of one image for the class the model predicts, batch axis squeezed."""
    x = transform(image).unsqueeze(0)
    y = int(model(x.to(device)).argmax())
    return explainer(x, [y]).squeeze()


def get_gradients_attribution_on_levels(images, model, explainer, transform, device, LEVELS):
    """Per image: the explanation's diagonal blocks, sum |gradient| per block, normalised to shares.
    The explainer runs once per image (WAM normalises by batch-global band maxima: batching would
    change the maps); the device maps are kept, one launch sums all blocks of all images and
    [N, LEVELS + 1] doubles come back."""
    kept = []
    for img in images:
        expl = get_explanations_for_image(img, model, explainer, transform, device, LEVELS)
        dev_map = getattr(explainer, "map_device", None)
        if dev_map is not None and dev_map.shape[0] == 1 and tuple(dev_map.shape[1:]) == tuple(np.shape(expl)):
            kept.append(dev_map[0].clone())
        else:  # an explainer without a device map: upload what it returned
            kept.append(_maps_dev(expl)[0])
    if not kept:
        return []
    for m in kept:
        assert m.dim() == 2 and m.shape[0] == m.shape[1], "grad_wam must be square"
    abs_sums, _, _ = _level_stats(torch.stack(kept).contiguous(), LEVELS, want_abs=True)
    return _shares(abs_sums.cpu().numpy())


def get_multiple_grad_attr(images, models, explainers, transform, device, LEVELS):
    """get_gradients_attribution_on_levels per (model, explainer) pair."""
    return [get_gradients_attribution_on_levels(images, m, e, transform, device, LEVELS)
            for m, e in zip(models, explainers)]


def get_mean_across_images(all_grads):
    """Mean share per level across images, for each model."""
    return [np.mean(np.array(grads), axis=0) for grads in all_grads]


# ------------------------------------------------------------------------------- mask agreement

def get_highest_percentage(gray, percentage):
    """bool mask of the pixels >= the int(len * percentage)-th largest value (index -1, the minimum,
    when that count is 0: everything is selected, as in the reference)."""
    host = not isinstance(gray, torch.Tensor)
    g = _flat_maps(gray[None])
    thr = _thresholds(g, [percentage])
    mask = (g[0] >= thr[0, 0]).reshape(tuple(gray.shape))
    return mask.cpu().numpy() if host else mask


def iou(mask1, mask2):
    """|both| / |either| of two bool masks on the host; 0 when neither selects anything."""
    either = np.logical_or(mask1, mask2).sum()
    return np.logical_and(mask1, mask2).sum() / either if either else 0


def _flat_maps(maps):
    """[M, ...] -> float64 device [M, len], contiguous."""
    g = _on_device(maps)
    return g.reshape(g.shape[0], -1).contiguous()


def _thresholds(flat, percentages):
    """[M, Q] device: per map the value at index int(len * p) - 1 of the descending sort (an order
    statistic: the reference's flat[argsort(flat)[::-1][int(len * p) - 1]])."""
    n = int(flat.shape[1])
    idx = [int(n * float(p)) - 1 for p in percentages]
    for i in idx:
        if i >= n or i < -n:
            raise IndexError("index %d is out of bounds for axis 0 with size %d" % (i, n))
    srt = torch.sort(flat, dim=1, descending=True).values
    return srt[:, [i % n for i in idx]].contiguous()


def _mask_iou_call(flat, thr):
    """One wam_mask_iou launch -> (rc, inter, uni) with int64 device tensors [Q, pairs]."""
    M, Q = int(thr.shape[0]), int(thr.shape[1])
    pairs = M * (M - 1) // 2
    inter = torch.empty((Q, pairs), dtype=torch.int64, device=flat.device)
    uni = torch.empty((Q, pairs), dtype=torch.int64, device=flat.device)
    with torch.cuda.device(flat.device):
        rc = lib.wam_mask_iou(M, Q, int(flat.shape[1]), ptr(flat), ptr(thr), ptr(inter), ptr(uni),
                              stream_of(flat.device))
    return rc, inter, uni


def _mask_counts(flat, thr):
    """(inter, uni) int64 numpy [Q, M (M - 1) / 2], pairs (i < j) in lexicographic order. One launch
    within the kernel's bounds; above them, blocks of maps are paired up and the percentages cut
    into chunks, each within the bounds."""
    M, Q = int(thr.shape[0]), int(thr.shape[1])
    rc, inter, uni = _mask_iou_call(flat, thr)
    if rc != _WAM_ERR_UNSUPPORTED:
        check(rc)
        return inter.cpu().numpy(), uni.cpu().numpy()
    pair_of = {}
    for i in range(M):
        for j in range(i + 1, M):
            pair_of[(i, j)] = len(pair_of)
    max_maps, max_q = _iou_limits()
    if M <= max_maps:
        groups = [list(range(M))]
    else:
        half = max_maps // 2
        blocks = [list(range(a, min(a + half, M))) for a in range(0, M, half)]
        groups = [blocks[a] + blocks[b] for a in range(len(blocks)) for b in range(a + 1, len(blocks))]
    inter_h = np.zeros((Q, len(pair_of)), dtype=np.int64)
    uni_h = np.zeros((Q, len(pair_of)), dtype=np.int64)
    for group in groups:
        sub = flat[group].contiguous()
        cols = [pair_of[(group[u], group[v])] for u in range(len(group)) for v in range(u + 1, len(group))]
        for q0 in range(0, Q, max_q):
            q1 = min(q0 + max_q, Q)
            rc, it, un = _mask_iou_call(sub, thr[group][:, q0:q1].contiguous())
            check(rc)
            inter_h[q0:q1, cols] = it.cpu().numpy()
            uni_h[q0:q1, cols] = un.cpu().numpy()
    return inter_h, uni_h


def mean_pairwise_iou(maps, percentages):
    """maps [M, ...] (host or device), percentages [Q] -> float64 [Q]: for each percentage the mean
    over the pairs (i < j) of iou(top-p mask of map i, top-p mask of map j). Thresholds are order
    statistics of a descending device sort, one wam_mask_iou launch counts every pair at every
    percentage, and the ratios are taken on the host from the integer counts."""
    flat = _flat_maps(maps)
    if flat.shape[0] < 2:
        raise ValueError("mean_pairwise_iou needs at least two maps")
    percentages = [float(p) for p in np.atleast_1d(np.asarray(percentages, dtype=np.float64))]
    inter, uni = _mask_counts(flat, _thresholds(flat, percentages))
    out = np.empty(len(percentages), dtype=np.float64)
    for q in range(len(percentages)):
        out[q] = np.mean([iq / uq if uq != 0 else 0 for iq, uq in zip(inter[q], uni[q])])
    return out


def _reprojection_dev(explanation, explainer, levels):
    """Device [S, S] float64: explainer.reproject_wam(explanation, levels).mean(axis=1) -- the planes
    added in order, then one division, as numpy reduces a non-contiguous axis. The notebook leaves
    reproject_wam's own approx_coeffs at its default, False, whatever the explainer was built with:
    the result has `levels` planes, the explainer's J of them filled (more raise, as in reproject_wam)."""
    avg = _maps_dev(explanation)
    if avg.shape[0] != 1:
        raise ValueError("get_grad_reprojection takes one map")
    n_out = int(levels)
    if explainer.J > n_out:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (n_out, n_out))
    sc = reproject_scales(avg, explainer.J, False)  # planes beyond these are zero in the reference's array
    acc = sc[0, 0].clone()
    for j in range(1, sc.shape[1]):
        acc += sc[0, j]
    return acc / torch.full((), float(n_out), dtype=torch.float64, device=acc.device)  # a true division


def get_grad_reprojection(explanation, explainer, levels, wavelet, method):
    return _reprojection_dev(explanation, explainer, levels).cpu().numpy()


def get_iou_between_wavelets(img, wavelets, p, *, model, transform, device, J, method):
    """Mean pairwise IoU of the top-p regions of one image's reprojected WAM under several wavelets.
    The notebook's globals (model, transform, device, LEVELS, METHOD) are keyword-only arguments; p
    may be a scalar (-> float) or a sequence (-> float64 [Q])."""
    from .wam_2D import WaveletAttribution2D

    reprojections = []
    for wave in wavelets:
        explainer = WaveletAttribution2D(model, wavelet=wave, J=J, method=method, mode="reflect")
        expl = get_explanations_for_image(img, model, explainer, transform, device, J)
        dev_map = explainer.map_device
        reprojections.append(_reprojection_dev(dev_map if dev_map is not None else expl, explainer, J))
    out = mean_pairwise_iou(torch.stack(reprojections), np.atleast_1d(p))
    return out if np.ndim(p) else out[0]
