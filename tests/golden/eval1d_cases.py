"""Shared definitions of the Eval1DWAM golden cases (inputs regenerated from numpy RandomState)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import testmodels  # noqa: E402
from tests.helpers import npz  # noqa: E402

GOLDENS = "eval1d_goldens.npz"
COMMON = dict(sample_rate=16000, n_mels=32, n_samples=2)
N_CLIPS = 2
N_ITERS = (4, 7)
TARGETS = ("wavelet", "melspec")
MODES = ("insertion", "deletion")
# rows of clip 0's n_iter = 4 wavelet-target model inputs that are stored
INPUT_ROWS = {"insertion": (1, 2, 4), "deletion": (0, 2, 3)}

CASES = {
    # the mel kernel path (n_fft a power of two), dyadic length: slices exactly n_i wide
    "k4096": dict(wavelet="haar", J=3, L=4096, n_fft=256, seed=421, y=[1, 4]),
    # bands 501, 501, 1001, 2001 against r = 0, 500, 1000, 2001, 4002: band 1 takes the pad column
    "pad4002": dict(wavelet="haar", J=3, L=4002, n_fft=256, seed=412, y=[2, 9]),
    # bands 501, 501, 1001, 2002 against r = 0, 500, 1001, 2002, 4004: band 1's slice starts one
    # slot before the band's own gradients, band 0 and band 1 share slot 500
    "shift4004": dict(wavelet="haar", J=3, L=4004, n_fft=256, seed=433, y=[2, 9]),
    # n_fft no power of two: the torch mel path; bands 258, 258, 515 against r = 0, 257, 515, 1030
    "torch1030": dict(wavelet="haar", J=2, L=1030, n_fft=200, seed=414, y=[3, 7]),
}


def make_inputs(case):
    rs = np.random.RandomState(case["seed"])
    x = rs.standard_normal((N_CLIPS, case["L"])).astype(np.float32)
    return torch.tensor(x), list(case["y"])


def make_model():
    return testmodels.TinyAudio()


def ctor_kw(case):
    return dict(wavelet=case["wavelet"], J=case["J"], method="smooth", mode="reflect", n_fft=case["n_fft"], **COMMON)


def thresholds(n_iter, length):
    """thr(m), m = 0 .. n_iter, of the reference's masks (src/evaluators.py:90-100)."""
    n_comp = int(length / n_iter)
    return [0] + [min(m * n_comp, length) for m in range(1, n_iter)] + [length]


def straddling_ties(values, n_iter):
    """Thresholds of an n_iter ranking of `values` (descending) that cut through a run of equal
    values: the masks then depend on the tie order of the sort."""
    v = np.sort(np.asarray(values).reshape(-1))[::-1]
    return [t for t in thresholds(n_iter, v.size) if 0 < t < v.size and v[t - 1] == v[t]]


# ------------------------------------------------------------------ readers of eval1d_goldens.npz
def cfg_of(case):
    return dict(wavelet=case["wavelet"], J=case["J"], n_fft=case["n_fft"], sample_rate=COMMON["sample_rate"],
                n_mels=COMMON["n_mels"])


def golden_grad_wams(name):
    d = npz(GOLDENS)
    J = CASES[name]["J"]
    return d[name + "_gw_mel"], [d["%s_gw_c%d" % (name, j)] for j in range(J + 1)]


def golden_masked(name, mode):
    """[clips, 5, K] float32: the n_iter = 4 masked coefficients the reference reconstructed."""
    d = npz(GOLDENS)
    coeffs = d[name + "_coeffs"]
    bits = np.unpackbits(d["%s_keep_%s" % (name, mode)], axis=-1)[..., :coeffs.shape[1]]
    return coeffs[:, None, :] * bits.astype(np.float32)
