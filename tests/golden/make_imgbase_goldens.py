"""EvalImageBaselines goldens: run the REFERENCE's own ``src/evaluators.py`` ``EvalImageBaselines`` and
``src/evaluation_helpers.py`` ``GradCAM`` / ``GradCAMPlusPlus`` / ``generate_images_baseline`` and store
what they return.

Run in the container that holds the reference checkout (it does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_imgbase_goldens.py

The reference imports packages that are absent offline; stand-ins are installed in ``sys.modules``
before it is imported (the pattern of ``make_eval1d_goldens.py``):

* ``pywt``, ``ptwt``, ``torchaudio(.transforms)``, ``pytorch_grad_cam(...)``, ``zennit.*``, ``lib.srd.*``,
  ``lib.wam_1D``, ``lib.wam_2D``, ``lib.network_architectures``, ``timm``, ``cv2``, ``librosa`` := modules whose
  every attribute is a placeholder (imported at module level, never on EvalImageBaselines' path);
* ``captum.attr.Saliency`` / ``IntegratedGradients`` := small stand-ins written for this generator (|input
  gradient| of the per-sample class score; zero-baseline riemann_trapezoid);
* ``torchvision.transforms`` := ``Compose``, ``Resize`` (Pillow's Image.resize, BILINEAR), ``ToTensor``,
  ``Normalize`` written for this generator;
* ``lib.helpers`` := the real ``src/helpers.py`` (for ``show``) when it imports with these placeholders,
  else a module with ``show`` restated from ``src/helpers.py:421-448``; which one was used is printed;
* ``src/evaluation_helpers.py`` is loaded under the name ``lib.evaluation_helpers``.

So these goldens pin the reference's own code -- the CAM weights, channel loop, normalisation and its
NaN map, generate_masks, the float64 mask product, normalize_data, the uint8 cast, softmax, AUC, the
mu-fidelity glue and its RNG draws -- and the real Pillow and torch (F.interpolate). They do not pin
captum or torchvision: those stay "parity unpinned", like cv2 and librosa elsewhere.

Stored (tests/golden/imgbase_cases.py; inputs are regenerated from RandomState):
  cam_<gradcam|gradcampp>_<layer>_<size>     the reference's maps [3, size, size] float32 (NaN maps included)
  img_<case>_<mode>                          generate_images_baseline's uint8 images (the case's stored masks;
                                             sha256 digests of them for the 224^2 case)
  <case>_<mode>_scores / _curves / _inputs   EvalImageBaselines with injected explanations: scores, curves,
                                             sha256 digests of the stored rows of image 0's model inputs
  mu_value / mu_bmask / mu_ys / mu_preds / mu_attrs   the mu-fidelity case (image by image)
  sal_expl, sal_<mode>_scores / _curves      the end-to-end saliency case

The generator fails unless no ranking behind a stored number has equal values straddling a threshold
and the mu-fidelity case's two lowest baseline-state probabilities are more than 1e-3 apart.
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REFERENCE = "/root/reference"

from tests.golden.imgbase_cases import (CAM_LAYERS, CAM_SIZES, CLASS_CASES, DIGESTED, GOLDENS, IMAGE_CASES,  # noqa: E402
                                        MODES, MU_CASE, SAL_CASE, cam_inputs, class_inputs, digest, image_case, make_model,
                                        straddling_ties)


def _placeholder_module(name):
    mod = types.ModuleType(name)
    mod.__getattr__ = lambda attr: type(attr, (), {})  # `from mod import Anything` succeeds
    mod.__all__ = []
    sys.modules[name] = mod
    return mod


# ------------------------------------------------------------------ stand-ins written for this generator
def _class_grads(model, x, target):
    x = x.detach().requires_grad_(True)
    out = model(x)
    return torch.autograd.grad(out.gather(1, target.long()[:, None]).sum(), x)[0]


class Saliency:
    def __init__(self, model):
        self.model = model

    def attribute(self, inputs, target=None, abs=True):
        g = _class_grads(self.model, inputs, target)
        return g.abs() if abs else g


class IntegratedGradients:
    def __init__(self, model):
        self.model = model

    def attribute(self, inputs, target=None, method="gausslegendre", n_steps=50, internal_batch_size=None,
                  return_convergence_delta=False):
        assert method == "riemann_trapezoid" and not return_convergence_delta
        steps = [1.0 / (n_steps - 1)] * n_steps
        steps[0] /= 2
        steps[-1] /= 2
        total = torch.zeros_like(inputs)
        for a, st in zip(np.linspace(0, 1, n_steps), steps):
            total = total + st * _class_grads(self.model, inputs * float(a), target)
        return total * inputs


class Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, im):
        for t in self.ts:
            im = t(im)
        return im


class Resize:
    def __init__(self, size):
        self.size = size

    def __call__(self, im):
        from PIL import Image
        h, w = self.size
        return im if im.size == (w, h) else im.resize((w, h), Image.BILINEAR)


class ToTensor:
    def __call__(self, im):
        a = np.asarray(im)
        a = a[:, :, None] if a.ndim == 2 else a
        return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean = torch.tensor(mean, dtype=torch.float32)[:, None, None]
        self.std = torch.tensor(std, dtype=torch.float32)[:, None, None]

    def __call__(self, t):
        return t.sub(self.mean).div(self.std)


def _show(img, p=False, inverse_c=False, smooth=1.2, plot=True, **kwargs):
    """src/helpers.py:421-448 for plot=False."""
    img = np.array(img, dtype=np.float32)
    if img.shape[0] == 1:
        img = img[0]
    elif img.shape[0] == 3:
        img = np.moveaxis(img, 0, 2)
    if img.shape[-1] == 1:
        img = img[:, :, 0]
    if img.max() > 1 or img.min() < 0:
        img -= img.min()
        img /= img.max()
    return img


def install_standins():
    for name in ("pywt", "ptwt", "torchaudio", "torchaudio.transforms", "pytorch_grad_cam", "pytorch_grad_cam.utils",
                 "pytorch_grad_cam.utils.model_targets", "zennit", "zennit.attribution", "zennit.composites",
                 "zennit.torchvision", "lib", "lib.srd", "lib.srd.util", "lib.srd.modules", "lib.srd.modules.resnet",
                 "lib.wam_1D", "lib.wam_2D", "lib.network_architectures", "timm", "cv2", "librosa", "captum",
                 "torchvision"):
        _placeholder_module(name)
    sys.modules["lib.wam_1D"].WaveletAttribution1D = type("WaveletAttribution1D", (), {})
    sys.modules["lib.wam_2D"].WaveletAttribution2D = type("WaveletAttribution2D", (), {})
    ca = types.ModuleType("captum.attr")
    ca.Saliency, ca.IntegratedGradients = Saliency, IntegratedGradients
    ca.GuidedBackprop = type("GuidedBackprop", (), {})
    sys.modules["captum.attr"] = ca
    tv = types.ModuleType("torchvision.transforms")
    tv.Compose, tv.Resize, tv.ToTensor, tv.Normalize = Compose, Resize, ToTensor, Normalize
    tv.__getattr__ = lambda attr: (lambda *a, **k: (lambda v: v))   # the transforms src/helpers.py builds but nobody runs
    sys.modules["torchvision.transforms"] = tv
    sys.modules["torchvision"].transforms = tv


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    sys.path.insert(0, REFERENCE)
    try:
        import matplotlib
        matplotlib.use("Agg")
        _load("lib.helpers", os.path.join(REFERENCE, "src", "helpers.py"))
        print("lib.helpers: the real src/helpers.py")
    except Exception as e:  # noqa: BLE001
        sys.modules.pop("lib.helpers", None)
        mod = types.ModuleType("lib.helpers")
        mod.show = _show
        sys.modules["lib.helpers"] = mod
        print("lib.helpers: show restated (src/helpers.py did not import: %s: %s)" % (type(e).__name__, e))
    helpers = _load("lib.evaluation_helpers", os.path.join(REFERENCE, "src", "evaluation_helpers.py"))
    return helpers, _load("reference_evaluators", os.path.join(REFERENCE, "src", "evaluators.py"))


def check_ties(what, values, n_iter):
    bad = straddling_ties(values, n_iter)
    assert not bad, "%s n_iter %d: a tie straddles thresholds %s" % (what, n_iter, bad)


def run_cams(helpers, out):
    nan_maps = 0
    for size in CAM_SIZES:
        x, y = cam_inputs(size)
        for layer in CAM_LAYERS:
            for name, cls in (("gradcam", helpers.GradCAM), ("gradcampp", helpers.GradCAMPlusPlus)):
                model = make_model()
                maps = cls(model, getattr(model, layer))(x.clone(), y)
                assert maps.dtype == np.float32 and maps.shape == (3, size, size)
                for m in maps:
                    assert np.isnan(m).all() or np.isfinite(m).all()
                    nan_maps += int(np.isnan(m).all())
                out["cam_%s_%s_%d" % (name, layer, size)] = maps
    assert nan_maps >= len(CAM_SIZES), "the all-NaN Grad-CAM of conv2 is gone from the cases"


def run_images(helpers, out):
    for name in IMAGE_CASES:
        img, expl, n_iter, rows = image_case(name)
        check_ties(name, expl, n_iter)
        for mode in MODES:
            ims = helpers.generate_images_baseline(img, expl, n_iter, mode)
            assert len(ims) == n_iter + 1
            got = [np.asarray(ims[m]) for m in rows]
            out["img_%s_%s" % (name, mode)] = np.stack([digest(a) for a in got] if name in DIGESTED else got)


def _evaluator(ev_mod, method, model, seen, **kw):
    model.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().cpu().numpy().copy()))
    return ev_mod.EvalImageBaselines(method, model, **kw)


def run_class(ev_mod, out):
    for name, case in CLASS_CASES.items():
        x, y, expl = class_inputs(case)
        for s in range(len(y)):
            check_ties("%s image %d" % (name, s), expl[s], case["n_iter"])
        seen = []
        ev = _evaluator(ev_mod, "saliency", make_model(), seen)
        ev.explanations = expl
        M = case["n_iter"] + 1
        for mode in MODES:
            del seen[:]
            scores = getattr(ev, mode)(x, y, n_iter=case["n_iter"])
            curves = ev.insertion_curves if mode == "insertion" else ev.deletion_curves
            inputs = np.concatenate(seen)
            assert inputs.shape == (len(y) * M, 3, 224, 224)
            out["%s_%s_scores" % (name, mode)] = np.array(scores)
            out["%s_%s_curves" % (name, mode)] = np.array(curves)
            out["%s_%s_inputs" % (name, mode)] = np.stack([digest(inputs[r]) for r in case["rows"]])


def run_mu(ev_mod, out):
    from scipy import stats
    case = MU_CASE
    x, y, expl = class_inputs(case)
    seen, pairs = [], []
    ev = _evaluator(ev_mod, "saliency", make_model(), seen, batch_size=case["batch_size"])
    ev.explanations = expl
    real = stats.spearmanr

    def spy(a, b):
        pairs.append((np.array(a), np.array(b)))
        return real(a, b)

    states = []
    inner = ev.compute_baseline_state

    def baseline_state(image, label, grid_size, batch_size, sample_size):
        del seen[:]
        mask = inner(image, label, grid_size, batch_size, sample_size)
        with torch.no_grad():
            p = torch.softmax(ev.model(torch.tensor(np.concatenate(seen))), dim=1)[:, label].numpy()
        states.append((mask, p))
        return mask

    ev.compute_baseline_state = baseline_state
    ev_mod.spearmanr = spy
    random.seed(case["pyseed"])
    try:
        mu = ev.mu_fidelity(x, y, grid_size=case["grid_size"], sample_size=case["sample_size"],
                            subset_size=case["subset_size"])
    finally:
        ev_mod.spearmanr = real
    assert len(pairs) == len(y) == len(states)
    for mask, p in states:
        lo = np.sort(p)[:2]
        assert lo[1] - lo[0] > 1e-3, "the two lowest baseline-state probabilities are %r" % (lo,)
    out["mu_value"] = np.array(mu)
    out["mu_bmask"] = np.stack([m for m, _ in states])
    out["mu_ys"] = np.stack([p for _, p in states])
    out["mu_preds"] = np.stack([a for a, _ in pairs])
    out["mu_attrs"] = np.stack([b for _, b in pairs])


def run_saliency(ev_mod, out):
    case = SAL_CASE
    x, y, _ = class_inputs(case)
    ev = _evaluator(ev_mod, "saliency", make_model(), [])
    for mode in MODES:
        scores = getattr(ev, mode)(x, y, n_iter=case["n_iter"])
        out["sal_%s_scores" % mode] = np.array(scores)
        out["sal_%s_curves" % mode] = np.array(ev.insertion_curves if mode == "insertion" else ev.deletion_curves)
    assert ev.explanations.dtype == np.float32
    for s in range(len(y)):
        check_ties("saliency image %d" % s, ev.explanations[s], case["n_iter"])
    out["sal_expl"] = ev.explanations


def main():
    install_standins()
    helpers, ev_mod = import_reference()
    torch.set_num_threads(min(8, os.cpu_count()))
    out = {}
    run_cams(helpers, out)
    run_images(helpers, out)
    run_class(ev_mod, out)
    run_mu(ev_mod, out)
    run_saliency(ev_mod, out)
    path = os.path.join(HERE, GOLDENS)
    np.savez_compressed(path, **out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
