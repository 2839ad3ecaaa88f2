"""Shared definitions of the EvalAudioBaselines golden cases (inputs regenerated from numpy RandomState)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import testmodels  # noqa: E402
from tests.golden.eval1d_cases import straddling_ties, thresholds  # noqa: E402,F401
from tests.helpers import npz  # noqa: E402

GOLDENS = "audiobase_goldens.npz"
SAMPLE_RATE = 16000
N_CLIPS = 2
MODES = ("insertion", "deletion")
GRAD_ITERS = (4, 7)     # n_iter of the stored saliency / integrated-gradients curves
CAM_ITERS = (2, 4)      # Grad-CAM is full of exact ReLU zeros: tie-free only at these, on the cam4096 case

# methods: per method the n_iter values whose curves are stored (): the explanation alone
CASES = {
    # the mel kernel path, T = 33 frames x 32 mels
    "k4096": dict(L=4096, n_fft=256, n_mels=32, seed=5, y=[1, 4],
                  methods={"saliency": GRAD_ITERS, "integratedgrad": GRAD_ITERS}),
    # the Grad-CAM curves: tie-free at n_iter 2 and 4 on both clips, fidelity gap 0.017
    "cam4096": dict(L=4096, n_fft=256, n_mels=32, seed=6, y=[2, 9], methods={"gradcam": CAM_ITERS}),
    # T = 158 frames x 128 mels = 20,224 cells: TinyAudio.conv's map is past wam_cam_maps' LDS bound
    "big20096": dict(L=20096, n_fft=256, n_mels=128, seed=5, y=[1, 4],
                     methods={"saliency": GRAD_ITERS, "integratedgrad": GRAD_ITERS, "gradcam": ()}),
    # n_fft no power of two: the torch mel path
    "torch1030": dict(L=1030, n_fft=200, n_mels=32, seed=5, y=[3, 7], methods={"saliency": GRAD_ITERS}),
}


class TinyAudioLayer(testmodels.TinyAudio):
    """TinyAudio with the ``layer`` attribute the reference's EvalAudioBaselines hands to Grad-CAM."""

    @property
    def layer(self):
        return self.conv


def make_inputs(case):
    rs = np.random.RandomState(case["seed"])
    x = rs.standard_normal((N_CLIPS, case["L"])).astype(np.float32)
    return torch.tensor(x), list(case["y"])


def make_model():
    return TinyAudioLayer()


def cfg_of(case):
    return dict(n_fft=case["n_fft"], sample_rate=SAMPLE_RATE, n_mels=case["n_mels"])


def golden(name, method, what):
    return npz(GOLDENS)["%s_%s_%s" % (name, method, what)]
