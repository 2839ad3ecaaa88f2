"""Eval1DWAM goldens: run the REFERENCE's own ``src/evaluators.py`` ``Eval1DWAM`` and store what it returns.

Run in the container that holds the reference checkout (it does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval1d_goldens.py

The reference imports packages that are absent offline; stand-ins are installed in ``sys.modules``
before it is imported (the pattern of ``make_glue_goldens.py``):

* ``ptwt``  := ``oracle.ptwt_torch``; ``pywt.waverec`` := ``oracle.dwt.waverec`` (float64 numpy);
* ``torchaudio.transforms`` := ``oracle.melspec``;
* ``torchvision.transforms``, ``captum.attr``, ``pytorch_grad_cam(.utils.model_targets)``,
  ``zennit.{attribution,composites,torchvision}``, ``lib.srd.*``, ``lib.helpers``, ``tqdm``, ``cv2``,
  ``librosa`` := modules whose every attribute is a placeholder (imported at module level by
  ``src/evaluators.py``, never on Eval1DWAM's path);
* ``src/evaluation_helpers.py`` is loaded under the name ``lib.evaluation_helpers``.

So these goldens pin Eval1DWAM's own glue -- ranking, thresholds, slice offsets, pad column, the
peak normalisation and its NaN row, softmax, AUC -- not ptwt, pywt or torchaudio.

Stored per case (tests/golden/eval1d_cases.py; inputs are regenerated from RandomState):
  gw_mel, gw_c<j>        the reference's grad_wams
  <target>_<mode>_n<k>_curves / _scores   for both targets, both modes, n_iter in {4, 7}
  coeffs, keep_<mode>    the n_iter = 4 masked coefficients the reference hands to pywt.waverec, as
                         the unmasked coefficients [clips, K] (band after band) and the packed bits of
                         masked != 0 [clips, 5, K]; the generator asserts that no coefficient is
                         exactly zero, so masked = coeffs * bits exactly
  inputs_<mode>          rows INPUT_ROWS[mode] of clip 0's n_iter = 4 wavelet-target model inputs
  ff_<target>, fid_<target>, fidlogits_<target>   faithfulness_of_spectra, input_fidelity and the
                         logits its arg-max was taken from

The tie condition: for every ranking behind a stored number (|coefficient gradient| per clip, the
signed mel gradient per clip; n_iter 2, 4 and 7) the values at ranks thr(m) - 1 and thr(m) differ
for every m, so that no mask depends on the tie order of numpy's (unstable) argsort. The generator
fails otherwise.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REFERENCE = "/root/reference"

from oracle import dwt, melspec, ptwt_torch  # noqa: E402
from tests.golden.eval1d_cases import (CASES, INPUT_ROWS, MODES, N_CLIPS, N_ITERS, TARGETS, ctor_kw,  # noqa: E402
                                       make_inputs, make_model, straddling_ties)

WAVEREC_CALLS = []


def _placeholder_module(name):
    mod = types.ModuleType(name)
    mod.__getattr__ = lambda attr: type(attr, (), {})  # `from mod import Anything` succeeds
    mod.__all__ = []
    sys.modules[name] = mod
    return mod


def install_standins():
    sys.modules["ptwt"] = ptwt_torch.as_module()
    pywt = types.ModuleType("pywt")

    def waverec(coeffs, wavelet):
        WAVEREC_CALLS.append([np.array(c) for c in coeffs])
        return dwt.waverec(coeffs, wavelet)

    pywt.waverec = waverec
    sys.modules["pywt"] = pywt
    ta = types.ModuleType("torchaudio")
    tat = types.ModuleType("torchaudio.transforms")
    tat.MelSpectrogram = melspec.MelSpectrogram
    tat.AmplitudeToDB = melspec.AmplitudeToDB
    ta.transforms = tat
    sys.modules["torchaudio"] = ta
    sys.modules["torchaudio.transforms"] = tat
    for name in ("torchvision", "torchvision.transforms", "captum", "captum.attr", "pytorch_grad_cam",
                 "pytorch_grad_cam.utils", "pytorch_grad_cam.utils.model_targets", "zennit", "zennit.attribution",
                 "zennit.composites", "zennit.torchvision", "lib.srd", "lib.srd.util", "lib.srd.modules",
                 "lib.srd.modules.resnet", "lib.helpers", "tqdm", "cv2", "librosa"):
        _placeholder_module(name)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    sys.path.insert(0, REFERENCE)
    _load("lib.evaluation_helpers", os.path.join(REFERENCE, "src", "evaluation_helpers.py"))
    return _load("reference_evaluators", os.path.join(REFERENCE, "src", "evaluators.py"))


def check_ties(name, mel, grads):
    for s in range(N_CLIPS):
        rankings = {"wavelet": np.abs(np.concatenate([g[s] for g in grads])), "melspec": mel[s]}
        for target, values in rankings.items():
            for n_iter in (2,) + tuple(N_ITERS):
                bad = straddling_ties(values, n_iter)
                assert not bad, "%s clip %d %s n_iter %d: a tie straddles thresholds %s" % (name, s, target, n_iter,
                                                                                           bad)


def run_case(ev_mod, name, case):
    x, y = make_inputs(case)
    model = make_model()
    seen = []
    model.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().cpu().numpy().copy()))
    kw = ctor_kw(case)
    ev = ev_mod.Eval1DWAM(model, wavelet=kw["wavelet"], J=kw["J"], method=kw["method"], mode=kw["mode"],
                          n_mels=kw["n_mels"], n_fft=kw["n_fft"], sample_rate=kw["sample_rate"],
                          n_samples=kw["n_samples"])
    out = {}
    for target in TARGETS:
        for mode in MODES:
            for n_iter in N_ITERS:
                del seen[:], WAVEREC_CALLS[:]
                scores = getattr(ev, mode)(x, y, target, n_iter)
                curves = ev.insertion_curves if mode == "insertion" else ev.deletion_curves
                key = "%s_%s_%s_n%d" % (name, target, mode, n_iter)
                out[key + "_scores"] = np.array(scores)
                out[key + "_curves"] = np.array(curves)
                if target == "wavelet" and n_iter == 4:
                    assert len(WAVEREC_CALLS) == N_CLIPS
                    masked = np.stack([np.concatenate(c, axis=1) for c in WAVEREC_CALLS])   # [clips, 5, K]
                    assert np.array_equal(masked, masked.astype(np.float32))
                    if mode == "insertion":
                        full = masked[:, n_iter]
                        assert (full != 0).all(), "a coefficient is exactly zero: the bits would lose its mask"
                        out[name + "_coeffs"] = full.astype(np.float32)
                    assert np.array_equal(masked, out[name + "_coeffs"][:, None, :] * (masked != 0))
                    out["%s_keep_%s" % (name, mode)] = np.packbits(masked != 0, axis=-1)
                    clip0 = seen[-N_CLIPS]   # the last forwards are the clips' (grad_wams' come first)
                    assert clip0.shape[0] == n_iter + 1
                    out["%s_inputs_%s" % (name, mode)] = clip0[list(INPUT_ROWS[mode]), 0]
    mel, grads = ev.grad_wams
    check_ties(name, mel, grads)
    out[name + "_gw_mel"] = mel
    for j, g in enumerate(grads):
        out["%s_gw_c%d" % (name, j)] = g
    for target in TARGETS:
        out["%s_ff_%s" % (name, target)] = np.array(ev.faithfulness_of_spectra(x, y, target))
        out["%s_fid_%s" % (name, target)] = np.array(ev.input_fidelity(x, y, target))
        out["%s_fidlogits_%s" % (name, target)] = np.array(ev.evaluate_auc(x, y, "insertion", target, 2, argmax=True))
    return out


def main():
    install_standins()
    ev_mod = import_reference()
    torch.set_num_threads(min(8, os.cpu_count()))
    out = {}
    for name, case in CASES.items():
        out.update(run_case(ev_mod, name, case))
        print(name, "ok")
    path = os.path.join(HERE, "eval1d_goldens.npz")
    np.savez_compressed(path, **out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
