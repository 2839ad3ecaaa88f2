"""EvalAudioBaselines goldens: run the REFERENCE's own ``src/evaluators.py`` ``EvalAudioBaselines`` and store
what it returns.

Run in the container that holds the reference checkout (it does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_audiobase_goldens.py

The reference imports packages that are absent offline; stand-ins are installed in ``sys.modules``
before it is imported (the pattern of ``make_eval1d_goldens.py`` / ``make_imgbase_goldens.py``):

* ``torchaudio.transforms`` := ``oracle.melspec`` (``MelSpectrogram``, ``AmplitudeToDB``);
* ``captum.attr.Saliency`` / ``IntegratedGradients`` := the small stand-ins of ``make_imgbase_goldens.py``
  (|input gradient| of the per-sample class score; zero-baseline riemann_trapezoid);
* ``pywt``, ``ptwt``, ``torchvision(.transforms)``, ``pytorch_grad_cam(...)``, ``zennit.*``, ``lib.srd.*``,
  ``lib.wam_1D``, ``lib.wam_2D``, ``lib.helpers``, ``tqdm``, ``cv2``, ``librosa`` := modules whose every
  attribute is a placeholder (imported at module level, never on EvalAudioBaselines' path);
* ``src/evaluation_helpers.py`` is loaded under the name ``lib.evaluation_helpers``.

So these goldens pin the reference's own code -- compute_melspec's layout, the choice and the arguments of
the method, GradCAM's weights, channel loop, normalisation and resize (the real torch F.interpolate),
generate_masks, the float64 mask product, softmax, AUC, the n_iter = 2 measures -- not captum or
torchaudio. The model is ``audiobase_cases.TinyAudioLayer``: TinyAudio with ``layer`` = its only conv.

Stored per case and method (tests/golden/audiobase_cases.py; inputs are regenerated from RandomState):
  <case>_<method>_expl                               compute_explanations
  <case>_<method>_<mode>_n<k>_scores / _curves       for the method's n_iter values of the case
  <case>_<method>_ff / _fid / _fidlogits             faithfulness_of_spectra, input_fidelity and the logits
                                                     its arg-max was taken from
(the explanation alone where the case lists no n_iter for the method). SmoothGrad has no goldens: the
reference's noise stream is unseeded.

The generator fails unless no ranking behind a stored number has equal values straddling a threshold
(n_iter 2 and the stored ones) and the top two logits behind every stored arg-max are at least 0.01
apart (100 bars of the device tests).
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import melspec  # noqa: E402
from tests.golden import make_imgbase_goldens as I  # noqa: E402
from tests.golden.audiobase_cases import (CASES, GOLDENS, MODES, N_CLIPS, SAMPLE_RATE, make_inputs,  # noqa: E402
                                          make_model, straddling_ties)

FIDELITY_GAP = 0.01


def install_standins():
    for name in ("pywt", "ptwt", "pytorch_grad_cam", "pytorch_grad_cam.utils", "pytorch_grad_cam.utils.model_targets",
                 "zennit", "zennit.attribution", "zennit.composites", "zennit.torchvision", "lib", "lib.srd",
                 "lib.srd.util", "lib.srd.modules", "lib.srd.modules.resnet", "lib.wam_1D", "lib.wam_2D", "lib.helpers",
                 "tqdm", "cv2", "librosa", "captum", "torchvision", "torchvision.transforms"):
        I._placeholder_module(name)
    sys.modules["lib.wam_1D"].WaveletAttribution1D = type("WaveletAttribution1D", (), {})
    sys.modules["lib.wam_2D"].WaveletAttribution2D = type("WaveletAttribution2D", (), {})
    ca = types.ModuleType("captum.attr")
    ca.Saliency, ca.IntegratedGradients = I.Saliency, I.IntegratedGradients
    ca.GuidedBackprop = type("GuidedBackprop", (), {})
    sys.modules["captum.attr"] = ca
    ta = types.ModuleType("torchaudio")
    tat = types.ModuleType("torchaudio.transforms")
    tat.MelSpectrogram = melspec.MelSpectrogram
    tat.AmplitudeToDB = melspec.AmplitudeToDB
    ta.transforms = tat
    sys.modules["torchaudio"] = ta
    sys.modules["torchaudio.transforms"] = tat


def import_reference():
    sys.path.insert(0, I.REFERENCE)
    I._load("lib.evaluation_helpers", os.path.join(I.REFERENCE, "src", "evaluation_helpers.py"))
    return I._load("reference_evaluators", os.path.join(I.REFERENCE, "src", "evaluators.py"))


def check_ties(what, expl, n_iters):
    for s in range(N_CLIPS):
        for n_iter in sorted(set((2,) + tuple(n_iters))):
            bad = straddling_ties(expl[s], n_iter)
            assert not bad, "%s clip %d n_iter %d: a tie straddles thresholds %s" % (what, s, n_iter, bad)


def run_case(ev_mod, name, case):
    x, y = make_inputs(case)
    out = {}
    for method, n_iters in case["methods"].items():
        ev = ev_mod.EvalAudioBaselines(method, make_model(), n_fft=case["n_fft"], sample_rate=SAMPLE_RATE,
                                       n_mels=case["n_mels"])
        key = "%s_%s_" % (name, method)
        expl = ev.compute_explanations(x, y)
        assert expl.dtype == np.float32 and expl.shape[0] == N_CLIPS and expl.shape[2] == case["n_mels"]
        out[key + "expl"] = expl
        if not n_iters:
            assert np.isfinite(expl).all()
            continue
        check_ties(key, expl, n_iters)
        for mode in MODES:
            for n_iter in n_iters:
                scores = getattr(ev, mode)(x, y, n_iter)
                assert scores[0].dtype == np.float32
                out["%s%s_n%d_scores" % (key, mode, n_iter)] = np.array(scores)
                out["%s%s_n%d_curves" % (key, mode, n_iter)] = np.array(ev.insertion_curves)  # sic: deletion too
        out[key + "ff"] = np.array(ev.faithfulness_of_spectra(x, y))
        out[key + "fid"] = np.array(ev.input_fidelity(x, y))
        logits = np.array(ev.evaluate_auc(x, y, "insertion", 2, argmax=True))
        top = np.sort(logits[:, 1:, :], axis=2)
        gap = float((top[:, :, -1] - top[:, :, -2]).min())
        assert gap >= FIDELITY_GAP, "%s: the top two logits behind an arg-max are %.4f apart" % (key, gap)
        assert np.array_equal(np.argmax(logits[:, 1:, :], axis=2), out[key + "fid"])
        out[key + "fidlogits"] = logits
        print("  %s ties ok, fidelity gap %.4f" % (key, gap))
    return out


def main():
    install_standins()
    ev_mod = import_reference()
    torch.set_num_threads(min(8, os.cpu_count()))
    out = {}
    for name, case in CASES.items():
        out.update(run_case(ev_mod, name, case))
        print(name, "ok")
    path = os.path.join(HERE, GOLDENS)
    np.savez_compressed(path, **out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
