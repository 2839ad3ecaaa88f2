"""Shared definitions of the EvalImageBaselines golden cases (inputs regenerated from numpy RandomState)."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import testmodels  # noqa: E402

GOLDENS = "imgbase_goldens.npz"
MODES = ("insertion", "deletion")

# ---- CAMs: GradCAM / GradCAMPlusPlus on both convolutions of TinySmooth2D. One image of every size has a
# conv2 Grad-CAM that is nowhere positive: the reference's 0 / 0, an all-NaN map.
CAM_SIZES = (32, 64)
CAM_LAYERS = ("conv", "conv2")
CAM_Y = (1, 3, 7)


def make_model():
    return testmodels.TinySmooth2D()


def cam_inputs(size):
    rs = np.random.RandomState(size)
    return torch.tensor(rs.uniform(size=(3, 3, size, size)).astype(np.float32)), list(CAM_Y)


# ---- generate_images_baseline: (H, W, n_iter, stored masks or None for all)
IMAGE_CASES = {
    "i15x17": (15, 17, 8, None),              # P = 255: no multiple of 4, n_comp = 31
    "i16x16": (16, 16, 7, None),              # n_iter does not divide P
    "i5x4": (5, 4, 32, None),                 # n_comp = 0: only the forced last mask keeps anything
    "i24x24": (24, 24, 128, (0, 1, 2, 64, 127, 128)),
    "i224": (224, 224, 64, (0, 1, 33, 64)),
}
DIGESTED = ("i224",)   # stored as one sha256 digest per image


def distinct_positive(rs, shape):
    """Strictly positive, pairwise distinct float64 values: no ranking depends on a tie order."""
    n = int(np.prod(shape))
    return ((rs.permutation(n) + 1.0) / n).reshape(shape)


def image_case(name):
    H, W, n_iter, rows = IMAGE_CASES[name]
    rs = np.random.RandomState(1000 + H * W + n_iter)
    img = rs.uniform(size=(H, W, 3)).astype(np.float32)
    return img, distinct_positive(rs, (H, W)), n_iter, (tuple(range(n_iter + 1)) if rows is None else rows)


# ---- the class with injected explanations: 224^2 (the fused output) and 64^2 (the resize path)
CLASS_CASES = {
    "c224": dict(size=224, n_iter=16, seed=511, y=[1, 3], rows=(0, 1, 9, 16)),
    "c64": dict(size=64, n_iter=8, seed=512, y=[2, 5], rows=(0, 3, 8)),
}


def class_inputs(case):
    rs = np.random.RandomState(case["seed"])
    S = case["size"]
    x = torch.tensor(rs.standard_normal((2, 3, S, S)).astype(np.float32))   # outside [0, 1]: show() rescales
    return x, list(case["y"]), distinct_positive(rs, (2, S, S))


# ---- mu-fidelity: one image pair at 64^2
MU_CASE = dict(size=64, seed=520, y=[1, 3], grid_size=8, sample_size=16, subset_size=20, batch_size=16, pyseed=5)

# ---- saliency end to end (explanations from the method itself)
SAL_CASE = dict(size=64, n_iter=8, seed=514, y=[4, 6])


def digest(a):
    """sha256 of an array's bytes as 32 uint8 (the large model inputs are stored as digests)."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def thresholds(n_iter, length):
    n_comp = int(length / n_iter)
    return [0] + [min(m * n_comp, length) for m in range(1, n_iter)] + [length]


def straddling_ties(values, n_iter):
    """Thresholds of an n_iter ranking of `values` (descending) that cut through a run of equal values."""
    v = np.sort(np.asarray(values).reshape(-1))[::-1]
    return [t for t in thresholds(n_iter, v.size) if 0 < t < v.size and v[t - 1] == v[t]]
