"""Plain-numpy restatement of the reference's Eval1DWAM (src/evaluators.py:39-306) and numpy
references of the three C-ABI entries behind wam_amd.evaluation.Eval1DWAM (TEST INFRASTRUCTURE).

The restatement takes grad_wams as an argument and runs the arithmetic the goldens were made with
(tests/golden/make_eval1d_goldens.py): analysis by oracle.ptwt_torch (float32, ptwt's default
mode 'reflect'), coeff * mask in float64, synthesis by oracle.dwt.waverec (float64), wf / wf.max() in
float64, a float32 cast, the dB mel spectrogram of oracle.melspec per waveform, the model on the CPU,
the host softmax and compute_auc. ``syn_dtype=np.float32`` runs the synthesis and the normalisation
in float32 instead -- the only arithmetic difference between the device pipeline and the reference
up to the mel front-end (the spread d32 of tests/test_gpu_eval1d.py).

The keyword arguments of ``Rules`` switch single reference rules off: the mutants the comparators of
tests/test_eval1d_ref.py must reject.

The C-ABI references (rank_mask_coeffs_ref, rank_mask_rows_ref, peak_normalize_ref) are written
from the contract sentences of include/wam_hip.h alone.
"""
import numpy as np
import torch

from oracle import dwt, melspec, ptwt_torch

F32, F64 = np.float32, np.float64

# The bar of the device pipeline against the goldens, on class probabilities (absolute):
# max(1e-4, 4 * d32). 1e-4 is the 2D evaluator's bar (tests/test_gpu_eval.py); d32 is the worst
# |delta p| of this restatement when its synthesis and normalisation run in float32 instead of
# float64 (measured over the golden cases by tests/test_eval1d_ref.py: 5.96e-8 = one float32 ulp of
# a probability in [0.5, 1)); the factor 4 covers the mel kernel's fp32 FFT against torch's STFT.
D32 = 5.96e-8
BAR = max(1e-4, 4 * D32)


class Rules:
    """The reference's rules; each flag set the other way is a mutant."""

    def __init__(self, offsets="waveform", pad_swapped=False, wavelet_abs=True, mel_abs=False, force_last=True,
                 silent="nan"):
        self.offsets = offsets          # 'waveform': r = int(L / 2^j); 'running': the bands' own running lengths
        self.pad_swapped = pad_swapped  # pad column 0 under insertion, 1 under deletion
        self.wavelet_abs = wavelet_abs
        self.mel_abs = mel_abs
        self.force_last = force_last
        self.silent = silent            # 'zero': a silent reconstruction is left as it is (Eval1DWAM(silent='zero'))


REFERENCE = Rules()


# ------------------------------------------------------------------------------ masks
def thresholds(n_iter, length):
    n_comp = int(length / n_iter)
    return [0] + [min(m * n_comp, length) for m in range(1, n_iter)] + [length]


def insertion_masks(order, n_iter, force_last=True):
    """[n_iter + 1, len] float64: mask m holds the first thr(m) entries of `order`."""
    masks = np.zeros((n_iter + 1, order.size))
    thr = thresholds(n_iter, order.size)
    if not force_last:
        thr[-1] = min(n_iter * int(order.size / n_iter), order.size)
    for m, t in enumerate(thr):
        masks[m, order[:t]] = 1
    return masks


def band_slices(length, levels, band_lens, offsets="waveform"):
    """(start, end) of every band's mask slice before clipping."""
    if offsets == "running":
        r = np.concatenate([[0], np.cumsum(band_lens)]).tolist()
    else:
        r = [0] + [int(length / 2 ** j) for j in range(levels, -1, -1)]
    return [(r[i], max(r[i + 1], n_i)) for i, n_i in enumerate(band_lens)]


def band_masks(masks, length, levels, band_lens, deletion, rules=REFERENCE):
    """The per-band masks [n_iter + 1, n_i] the reference multiplies into the coefficients."""
    out = []
    pad = 0.0 if deletion else 1.0
    if rules.pad_swapped:
        pad = 1.0 - pad
    for (start, end), n_i in zip(band_slices(length, levels, band_lens, rules.offsets), band_lens):
        m = masks[:, start:end]
        if m.shape[1] != n_i:
            m = np.pad(m, ((0, 0), (0, 1)), mode="constant", constant_values=pad)
        if m.shape[1] != n_i:
            raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,%d)"
                             % (n_i, m.shape[0], m.shape[1]))
        out.append(m)
    return out


# ------------------------------------------------------------------------------ front-end
def _waverec32(coeffs, wavelet):
    """oracle.dwt.waverec's 1D recursion with every value and filter tap in float32."""
    _, _, rec_lo, rec_hi = (f.astype(F32) for f in dwt.filter_bank(wavelet))
    L = len(rec_lo)
    p = (2 * L - 3) // 2
    a = coeffs[0].astype(F32)
    for c_pos, d in enumerate(coeffs[1:]):
        d = d.astype(F32)
        m = a.shape[-1]
        y = np.zeros(a.shape[:-1] + (2 * m - 2 + L,), dtype=F32)
        for k in range(L):
            y[..., k:k + 2 * m - 1:2] += rec_lo[k] * a + rec_hi[k] * d
        extra = c_pos < len(coeffs) - 2 and coeffs[c_pos + 2].shape[-1] == y.shape[-1] - 2 * p - 1
        a = y[..., p:y.shape[-1] - p - (1 if extra else 0)]
    return a


def compute_melspec(waves, n_fft, sample_rate, n_mels):
    """lib/wam_1D.py:194-219: per waveform, [N, 1, T, n_mels] float32 torch."""
    to_db = melspec.AmplitudeToDB()
    mel = melspec.MelSpectrogram(sample_rate=sample_rate, n_fft=n_fft, n_mels=n_mels)
    return torch.stack([to_db(mel(w)).T.squeeze(-1).unsqueeze(0) for w in torch.as_tensor(waves)])


def peak_normalize(rec, silent="nan"):
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.array([wf if (silent == "zero" and wf.max() == 0) else wf / wf.max() for wf in rec])
    return out


def wavelet_inputs(x_s, gradients, sample, mode, n_iter, cfg, rules=REFERENCE, syn_dtype=F64):
    """auc_from_wavelet (:56-143) -> (masked coefficients [n_iter + 1, K] float64, band after band;
    model inputs [n_iter + 1, 1, T, n_mels] float32 torch)."""
    coeffs = [c.numpy() for c in ptwt_torch.wavedec(torch.as_tensor(x_s), cfg["wavelet"], level=cfg["J"])]
    g = np.concatenate([b[sample] for b in gradients])
    order = np.argsort(np.abs(g) if rules.wavelet_abs else g)[::-1]
    ins = insertion_masks(order, n_iter, rules.force_last)
    deletion = mode == "deletion"
    masks = band_masks(1.0 - ins if deletion else ins, x_s.shape[0], cfg["J"], [c.shape[0] for c in coeffs], deletion,
                       rules)
    filtered = [c * m for c, m in zip(coeffs, masks)]
    if syn_dtype == F64:
        rec = dwt.waverec(filtered, cfg["wavelet"])
    else:
        rec = _waverec32(filtered, cfg["wavelet"])
    wave = peak_normalize(rec, rules.silent).astype(F32)
    return np.concatenate(filtered, axis=1), compute_melspec(wave, cfg["n_fft"], cfg["sample_rate"], cfg["n_mels"])


def melspec_inputs(mel_grad, source, mode, n_iter, rules=REFERENCE):
    """auc_from_melspec (:145-176) with generate_masks (src/evaluation_helpers.py:455-499)."""
    v = np.abs(mel_grad) if rules.mel_abs else mel_grad
    order = np.argsort(v, axis=None)[::-1]
    ins = insertion_masks(order, n_iter, rules.force_last).reshape((n_iter + 1,) + mel_grad.shape)
    return torch.tensor((1.0 - ins if mode == "deletion" else ins) * source).float().unsqueeze(1)


# ------------------------------------------------------------------------------ the class
def compute_auc(probs):
    return sum(probs) / (np.max(probs) * len(probs))


def evaluate_auc(model, x, y, grad_wams, mode, target, n_iter, cfg, rules=REFERENCE, syn_dtype=F64, keep=None):
    """evaluate_auc (:178-235) -> (scores, curves, raw logits); keep: a dict that receives the
    masked coefficients and model inputs per clip."""
    x = np.asarray(x, dtype=F32)
    mel_grads, gradients = grad_wams
    source = compute_melspec(x, cfg["n_fft"], cfg["sample_rate"], cfg["n_mels"]).squeeze(1).numpy()
    scores, curves, raw = [], [], []
    for s in range(x.shape[0]):
        if target == "melspec":
            masked, inputs = None, melspec_inputs(mel_grads[s], source[s], mode, n_iter, rules)
        else:
            masked, inputs = wavelet_inputs(x[s], gradients, s, mode, n_iter, cfg, rules, syn_dtype)
        with torch.no_grad():
            preds = model(inputs).cpu().numpy()
        with np.errstate(invalid="ignore"):
            probs = np.exp(preds) / np.sum(np.exp(preds), axis=1, keepdims=True)
            p = probs[:, y[s]]
            scores.append(compute_auc(p))
        curves.append(p)
        raw.append(preds)
        if keep is not None:
            keep.setdefault("masked", []).append(masked)
            keep.setdefault("inputs", []).append(inputs.numpy())
    return scores, curves, raw


def faithfulness_of_spectra(model, x, y, grad_wams, target, cfg, rules=REFERENCE, syn_dtype=F64):
    _, curves, _ = evaluate_auc(model, x, y, grad_wams, "deletion", target, 2, cfg, rules, syn_dtype)
    curves = np.array(curves)
    return (curves[:, 0] - curves[:, 1]).tolist()


def input_fidelity(model, x, y, grad_wams, target, cfg, rules=REFERENCE, syn_dtype=F64):
    _, _, raw = evaluate_auc(model, x, y, grad_wams, "insertion", target, 2, cfg, rules, syn_dtype)
    return np.argmax(np.array(raw)[:, 1:, :], axis=2).tolist()


# ------------------------------------------------------------------------------ C-ABI references
def _thr(m, n_iter, n_comp, rank_len):
    if m == 0:
        return 0
    if m >= n_iter:
        return rank_len
    return min(m * n_comp, rank_len)


def _keep(rank_of_value, n_iter, n_comp, rank_len, deletion):
    """[n_iter + 1, ...] float32 of 1.0 / 0.0: (rank < thr(m)) != (deletion != 0)."""
    thr = np.array([_thr(m, n_iter, n_comp, rank_len) for m in range(n_iter + 1)], dtype=np.int64)
    thr = thr.reshape((-1,) + (1,) * rank_of_value.ndim)
    return ((rank_of_value[None].astype(np.int64) < thr) != bool(deletion)).astype(F32)


def rank_mask_coeffs_ref(band_off, sets, coeffs, rank, pos, n_iter, n_comp, deletion):
    """wam_rank_mask_coeffs: coeffs flat band-major over `sets` items, rank [sets, rank_len], pos [K]
    -> flat band-major over sets * (n_iter + 1) items, item (s, m) = s * (n_iter + 1) + m."""
    coeffs = np.asarray(coeffs, dtype=F32)
    rank_len = rank.shape[1]
    M = n_iter + 1
    out = np.empty(sets * M * band_off[-1], dtype=F32)
    pos = np.asarray(pos, dtype=np.int64)
    pad = (pos < 0) | (pos >= rank_len)          # the pad column (any value outside [0, rank_len) reads as -1)
    for b in range(len(band_off) - 1):
        n_b = band_off[b + 1] - band_off[b]
        p = pos[band_off[b]:band_off[b + 1]]
        is_pad = pad[band_off[b]:band_off[b + 1]]
        for s in range(sets):
            c = coeffs[sets * band_off[b] + s * n_b:sets * band_off[b] + (s + 1) * n_b]
            k = _keep(rank[s][np.where(is_pad, 0, p)], n_iter, n_comp, rank_len, deletion)
            k[:, is_pad] = 0.0 if deletion else 1.0
            o = sets * M * band_off[b] + s * M * n_b
            out[o:o + M * n_b] = (c[None, :] * k).reshape(-1)
    return out


def rank_mask_rows_ref(src, rank, n_iter, n_comp, deletion):
    """wam_rank_mask_rows: src [sets, len], rank [sets, len] -> [sets, n_iter + 1, len]."""
    src = np.asarray(src, dtype=F32)
    return np.stack([src[s][None, :] * _keep(rank[s], n_iter, n_comp, src.shape[1], deletion)
                     for s in range(src.shape[0])])


def peak_normalize_ref(x, zero_silent):
    """wam_peak_normalize: x [rows, len] float32 -> (out float32, silent int32)."""
    x = np.asarray(x, dtype=F32)
    mx = x.max(axis=1)
    silent = (mx == 0).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = x / mx[:, None]                    # float32 / float32: IEEE fp32 division
    if zero_silent:
        out[silent == 1] = x[silent == 1]
    return out, silent


def assert_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(ref, dtype=F32)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    bad &= ~(np.isnan(got) & np.isnan(ref))      # any NaN equals any NaN
    assert not bad.any(), "%s: %d of %d values differ in bits, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], ref[bad][0])
