"""Plain-numpy restatement of the reference's WAMAnalyzer2D (src/analyzers.py:16-203) and its helpers
(src/analyzers_helpers.py:6-134), and numpy references of the C-ABI entries behind
wam_amd.analysis.WAMAnalyzer2D (TEST INFRASTRUCTURE).

The restatement runs the transform with oracle.dwt (float64, pywt's default mode 'symmetric') where
the reference runs pywt in float32 on show()'s float32 image; its images are cast to float32 at the
end. D32 is the distance that leaves against the goldens (tests/test_analyzer_ref.py measures it).
The keyword arguments of ``Rules`` switch single reference rules off: the mutants the comparators
of tests/test_analyzer_ref.py must reject.

The C-ABI references (threshold_mask_coeffs_ref, quantize_ref) are written from the contract
sentences of include/wam_hip.h alone.
"""
import numpy as np
import torch

from oracle import dwt

F32, F64 = np.float32, np.float64
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# Worst max |restatement - golden| / max |golden| over the float images of the goldens (partial images and
# level images, 32^2 and 64^2), float64 oracle.dwt against float32 pywt: measured 4.77e-7 (the 64^2 partial image at q = 0; 1.0e-7 to 3.6e-7 elsewhere) by
# tests/test_analyzer_ref.py::test_float_images_within_d32, which holds the restatement to this value.
# The device tests allow 4 * D32 (the device sums each Haar level in another order than pywt).
D32 = 4.8e-7
CAP = 1e-3   # share of uint8 pixels that may sit one (circular) grey level apart: tests/test_gpu_eval.py's cap


class Rules:
    """The reference's rules; each flag set the other way is a mutant."""

    def __init__(self, ge=True, layout="pywt", level_shift=0, level_min="array", quant="quirk", cast="wrap",
                 lerp_second=True):
        self.ge = ge                    # mask = map >= t; False: map > t
        self.layout = layout            # 'pywt': cH bottom-left, cV top-right; 'mosaic': swapped
        self.level_shift = level_shift  # 1: every level region taken one level coarser
        self.level_min = level_min      # 'array': min over the whole entry, zeros included; 'region': over the region
        self.quant = quant              # 'quirk': ((x - mn) / mx - mn) * 255; 'minmax'
        self.cast = cast                # 'wrap': low 8 bits of the truncated value; 'saturate': clipped to [0, 255]
        self.lerp_second = lerp_second  # False: a + (b - a) * g for every g


REFERENCE = Rules()


# ------------------------------------------------------------------------------ quantile
def quantile(values, q, rules=REFERENCE):
    """np.quantile(values, q), method 'linear', restated: virtual index (n - 1) * q, the two order
    statistics around it, numpy's _lerp."""
    s = np.sort(np.asarray(values, dtype=F64).reshape(-1))
    vi = (s.size - 1) * F64(q)
    lo = int(np.floor(vi))
    g = vi - lo
    a, b = s[lo], s[min(lo + 1, s.size - 1)]
    d = b - a
    if rules.lerp_second and g >= 0.5:
        return b - d * (1 - g)
    return a + d * g


# ------------------------------------------------------------------------------ pywt's array
def to_array(coeffs, layout="pywt"):
    """pywt.coeffs_to_array of a wavedec2 list [cA, (cH, cV, cD) coarsest first, ...] and the slices to
    undo it. layout 'mosaic' puts cH top-right and cV bottom-left (the WAM mosaic: the mutant)."""
    ah, aw = coeffs[0].shape
    H = ah + sum(lv[2].shape[0] for lv in coeffs[1:])
    W = aw + sum(lv[2].shape[1] for lv in coeffs[1:])
    arr = np.zeros((H, W), dtype=coeffs[0].dtype)
    arr[:ah, :aw] = coeffs[0]
    slices = [(slice(0, ah), slice(0, aw))]
    for ch, cv, cd in coeffs[1:]:
        dh, dw = cd.shape
        below = (slice(ah, ah + ch.shape[0]), slice(0, ch.shape[1]))
        right = (slice(0, cv.shape[0]), slice(aw, aw + cv.shape[1]))
        if layout == "mosaic":
            below = (slice(ah, ah + cv.shape[0]), slice(0, cv.shape[1]))
            right = (slice(0, ch.shape[0]), slice(aw, aw + ch.shape[1]))
            s = (right, below, (slice(ah, ah + dh), slice(aw, aw + dw)))
        else:
            s = (below, right, (slice(ah, ah + dh), slice(aw, aw + dw)))
        for band, sl in zip((ch, cv, cd), s):
            arr[sl] = band
        slices.append(s)
        ah, aw = ah + dh, aw + dw
    return arr, slices


def from_array(arr, slices):
    return [arr[slices[0]]] + [tuple(arr[sl] for sl in s) for s in slices[1:]]


def masked_image(img, mask, J, wavelet, rules=REFERENCE):
    """Every channel of img [S, S, 3]: wavedec2 -> array * mask -> waverec2; float64 [S, S, 3]."""
    chans = []
    for c in range(img.shape[2]):
        arr, sl = to_array(dwt.wavedec2(img[:, :, c].astype(F64), wavelet, J, mode="symmetric"), rules.layout)
        if arr.shape != mask.shape:
            raise ValueError("operands could not be broadcast together with shapes (%d,%d) (%d,%d)"
                             % (arr.shape + mask.shape))
        chans.append(dwt.waverec2(from_array(arr * mask, sl), wavelet))
    return np.stack(chans, axis=2)


def partial_image(img, grad_wam, q, J, wavelet="haar", rules=REFERENCE):
    """generate_partial_image: (image float32, mask * grad_wam, the threshold)."""
    t = quantile(grad_wam, q, rules)
    mask = grad_wam >= t if rules.ge else grad_wam > t
    return masked_image(img, mask, J, wavelet, rules).astype(F32), mask * grad_wam, t


# ------------------------------------------------------------------------------ levels
def level_edges(size, J):
    return [int(size / 2 ** j) for j in range(J + 1)]


def level_regions(size, J, shift=0):
    """[J + 1, size, size] bool: entry j < J = the blocks [s:e, s:e], [s:e, :s], [:s, s:e] with s =
    int(size / 2^(j + 1)), e = int(size / 2^j); entry J = [:a, :a], a = int(size / 2^J)."""
    reg = np.zeros((J + 1, size, size), dtype=bool)
    for j in range(J):
        s, e = int(size / 2 ** (j + 1 + shift)), int(size / 2 ** (j + shift))
        reg[j, s:e, s:e] = True
        reg[j, s:e, :s] = True
        reg[j, :s, s:e] = True
    a = int(size / 2 ** (J + shift))
    reg[J, :a, :a] = True
    return reg


def levelized_masks(grad_wam, J, rules=REFERENCE):
    return level_regions(grad_wam.shape[0], J, rules.level_shift) * np.asarray(grad_wam, dtype=F64)[None]


def disentangled(grad_wam, img, J, eps=0.1, wavelet="haar", rules=REFERENCE):
    """generate_disentangled_images: (partial_images [J + 1, S, S, 3] float64 holding float32 values,
    filtered_masks [J + 1, S, S])."""
    filtered = levelized_masks(grad_wam, J, rules)
    regions = level_regions(grad_wam.shape[0], J, rules.level_shift)
    out = np.zeros((J + 1,) + img.shape)
    for l in range(J + 1):
        lowest = filtered[l].min() if rules.level_min == "array" else filtered[l][regions[l]].min()
        rec = masked_image(img, filtered[l] > lowest + eps, J, wavelet, rules)
        out[l] = np.clip(rec, 0, 255).astype(F32)
    return out, filtered


# ------------------------------------------------------------------------------ quantisation
def wrap_u8(s):
    """numpy's float32 -> uint8 cast as x86 does it: truncation toward zero to int32, the low 8 bits
    kept; NaN, infinities and values beyond int32 give 0."""
    s = np.asarray(s, dtype=F32)
    ok = np.abs(s) < F32(2147483648.0)   # False for NaN
    t = np.trunc(np.where(ok, s, F32(0))).astype(np.int64)
    return (t & 255).astype(np.uint8)


def quantize(image, rules=REFERENCE):
    """image float32 (any layout, one image) -> uint8: the analyzer's ((x - mn) / mx - mn) * 255 in float32,
    numpy's order, then the wrapping cast."""
    x = np.asarray(image, dtype=F32)
    mn, mx = x.min(), x.max()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if rules.quant == "minmax":
            s = ((x - mn) / (mx - mn)) * F32(255)
        else:
            s = ((x - mn) / mx - mn) * F32(255)
    assert s.dtype == F32
    if rules.cast == "saturate":
        return np.clip(np.trunc(np.nan_to_num(s, nan=0.0)), 0, 255).astype(np.uint8)
    return wrap_u8(s)


def circular(a, b):
    """Circular grey-level distance min(d, 256 - d) of two uint8 arrays."""
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    return np.minimum(d, 256 - d)


def float_distance(got, want):
    """max |got - want| relative to max |want|: the measure D32 is stated in."""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape
    return float(np.abs(got - want).max() / np.abs(want).max())


def u8_compare(got, want):
    """(largest circular grey-level distance, share of pixels with a non-zero distance)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    d = circular(got, want)
    return int(d.max()), float((d > 0).mean())


def to_input(u8):
    """Resize((224, 224)) (real Pillow; the identity at 224 x 224) + ToTensor + Normalize of one uint8 HWC image."""
    from oracle import evaluation_ref as E
    return E.to_input(u8)


def show(img):
    from oracle import evaluation_ref as E
    return E.show(img)


# ------------------------------------------------------------------------------ the class
def isolate_necessary_components(model, x, y, grad_wams, qs, mode, J, wavelet="haar", rules=REFERENCE):
    """src/analyzers.py:94-203 with the default transform: (outs, the quantiles appended). The images of
    the tuples are uint8 HWC arrays (what the reference wraps in PIL.Image.fromarray)."""
    if mode is None:
        raise ValueError
    if mode == "deletion":
        assert qs[0] <= qs[1]
    if mode == "insertion":
        assert qs[0] >= qs[1]
    outs, appended = [], []
    for i in range(x.shape[0]):
        img = show(x[i])
        images, masks = [], []
        for q in qs:
            image, mask, _ = partial_image(img, grad_wams[i], q, J, wavelet, rules)
            images.append(quantize(image, rules))
            masks.append(mask)
        with torch.no_grad():
            preds = model(torch.stack([to_input(im) for im in images])).numpy()
        probs = np.exp(preds) / np.sum(np.exp(preds), axis=1, keepdims=True)
        hits = np.where(np.argmax(preds, axis=1) == y[i])[0]
        if not len(hits):
            outs.append(((None, None, None), None, grad_wams[i], (None, np.nan)))
            continue
        ci = hits[-1] if mode == "deletion" else hits[0]
        appended.append(qs[ci])
        outs.append(((images[0], images[ci], images[-1]), masks[ci], grad_wams[i], (probs, ci)))
    return outs, appended


# ------------------------------------------------------------------------------ C-ABI references
def threshold_mask_coeffs_ref(off, images, channels, coeffs, pos, size, wam, n_thr, thr, thr_stride, level_mode=0,
                              edges=None, strict=0):
    """wam_threshold_mask_coeffs: coeffs flat band-major over images * channels planes, pos [K] int32,
    wam [images, size * size] float64, thr flat float64 (row n at n * thr_stride) -> flat band-major
    float32 over images * n_thr * channels planes, plane (n, q, c) = (n * n_thr + q) * channels + c."""
    nb = len(off) - 1
    P, PO = images * channels, images * n_thr * channels
    out = np.empty(PO * off[nb], dtype=F32)
    wam = np.asarray(wam, dtype=F64).reshape(images, size * size)
    thr = np.asarray(thr, dtype=F64).reshape(-1)
    for b in range(nb):
        bn = off[b + 1] - off[b]
        p = np.asarray(pos[off[b]:off[b + 1]], dtype=np.int64)
        inside = (p >= 0) & (p < size * size)
        pc = np.where(inside, p, 0)
        src = coeffs[P * off[b]:P * off[b + 1]].reshape(images, channels, bn)
        dst = out[PO * off[b]:PO * off[b + 1]].reshape(images, n_thr, channels, bn)
        for n in range(images):
            v = wam[n, pc]
            for q in range(n_thr):
                vq = v
                if level_mode:
                    m = np.maximum(pc // size, pc % size)
                    reg = m < edges[n_thr - 1] if q == n_thr - 1 else (m >= edges[q + 1]) & (m < edges[q])
                    vq = np.where(reg, v, 0.0)
                t = thr[n * thr_stride + q]
                with np.errstate(invalid="ignore"):
                    keep = ((vq > t) if strict else (vq >= t)) & inside
                dst[n, q] = src[n] * np.where(keep, F32(1), F32(0))[None, :]
    return out


def quantize_ref(rec, rule, mean=None, std=None):
    """wam_quantize_normalize_ex: rec [images, channels, plane] float32 -> (u8 [images, channels, plane],
    out float32 or None without mean / std)."""
    rec = np.asarray(rec, dtype=F32)
    u8 = np.empty(rec.shape, dtype=np.uint8)
    for i, x in enumerate(rec):
        mn, mx = x.min(), x.max()
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if rule == 0:
                s = ((x - mn) / (mx - mn)) * F32(255)
                u8[i] = np.where(np.isnan(s), 0, np.trunc(np.nan_to_num(s, nan=0.0))).astype(np.uint8)
            else:
                s = ((x - mn) / mx - mn) * F32(255)
                u8[i] = wrap_u8(s)
    if mean is None:
        return u8, None
    m = np.asarray(mean, dtype=F32)[None, :, None]
    sd = np.asarray(std, dtype=F32)[None, :, None]
    return u8, ((u8.astype(F32) / F32(255) - m) / sd).astype(F32)


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    same = got.view(np.uint8) == want.view(np.uint8)
    assert same.all(), "%s: %d of %d bytes differ" % (what, (~same).sum(), same.size)
