"""EvalAudioBaselines and wam_cam_maps_tiled without a device: the exports, the host argument checks of the
tiled Grad-CAM entry, the constructor's errors, and the numpy restatement (tests/audiobase_ref.py) against
the goldens made by the reference's own class (tests/golden/audiobase_goldens.npz). CPU only.

The restatement and the generator run the same CPU model and the same oracle mel front-end; what differs
is the summation order of the methods (float64 sums in tests/baselines_ref.py where the reference and its
stand-ins add float32 tensors), so explanations are held to 1e-4 of their maximum and curves, scores and
faithfulness to 1e-4 (the project's bar for quantities that pass through the model). Measured here
(each test prints its figure): explanations 0 (saliency: the same operations), 2.03e-7 (integrated
gradients), 1.19e-7 (Grad-CAM, both shapes); curves, scores and faithfulness on the golden explanations 0.
"""
import ctypes

import numpy as np
import pytest

from tests import audiobase_ref as A
from tests import eval1d_ref as R1
from tests.baselines_ref import cam_distance
from tests.golden import audiobase_cases as C

BAR = 1e-4


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def _distance(got, ref, method):
    return cam_distance(got, ref) if method == "gradcam" else _rel(got, ref)


# ------------------------------------------------------------------------------ exports, host checks
def test_exports():
    import wam_amd
    import wam_amd.evaluation
    from wam_amd import _lib
    assert wam_amd.EvalAudioBaselines is wam_amd.evaluation.EvalAudioBaselines
    assert "EvalAudioBaselines" in wam_amd.__all__
    assert _lib.lib.wam_cam_maps_tiled.restype is ctypes.c_int
    assert _lib.lib.wam_cam_maps_tiled_ws_bytes.restype is ctypes.c_int64
    header = open(_lib.HEADER_PATH).read()
    assert "int wam_cam_maps_tiled(" in header and "int64_t wam_cam_maps_tiled_ws_bytes(" in header


def test_tiled_cam_host_argument_checks():
    """Every one of these returns before anything touches a device."""
    from wam_amd._lib import lib
    p = ctypes.c_void_p(4096)   # never dereferenced: the checks fail first
    ws_bytes = lib.wam_cam_maps_tiled_ws_bytes(1, 4, 157, 128)
    call = lambda images=1, K=4, h=157, w=128, act=p, grad=p, oh=157, ow=128, out=p, ws=p, n=ws_bytes: (  # noqa: E731
        lib.wam_cam_maps_tiled(images, K, h, w, act, grad, 0, oh, ow, out, ws, n, None))
    assert call(K=0) == 1
    assert call(h=0) == 1 and call(ow=0) == 1 and call(images=-1) == 1
    assert call(act=None) == 1 and call(grad=None) == 1 and call(out=None) == 1
    assert call(ws=None) == 1
    assert call(n=ws_bytes - 1) == 1                 # a short workspace
    assert call(ws=ctypes.c_void_p(4100)) == 1       # not 8-byte aligned
    assert call(h=65536, w=65536, n=1 << 62) == 1    # h * w above INT32_MAX
    assert call(images=0, ws=None, n=0) == 0         # nothing to do


def test_tiled_cam_workspace_formula():
    """8 * images * (2 * K * S + h * w + 2 * T), S = min(64, ceil(h * w / 1024)), T = ceil(h * w / 1024)."""
    from wam_amd._lib import lib
    for images, K, h, w in ((2, 4, 157, 128), (1, 3, 150, 131), (1, 19500, 2, 2), (3, 16, 431, 128), (0, 1, 1, 1)):
        T = -(-h * w // 1024)
        assert lib.wam_cam_maps_tiled_ws_bytes(images, K, h, w) == 8 * images * (2 * K * min(64, T) + h * w + 2 * T)
    assert lib.wam_cam_maps_tiled_ws_bytes(1, 0, 4, 4) < 0
    assert lib.wam_cam_maps_tiled_ws_bytes(-1, 1, 4, 4) < 0
    assert lib.wam_cam_maps_tiled_ws_bytes(1, 1, 65536, 65536) < 0


def test_constructor_errors():
    import testmodels
    from wam_amd import EvalAudioBaselines
    with pytest.raises(ValueError, match="occlusion"):
        EvalAudioBaselines("occlusion", C.make_model())
    with pytest.raises(ValueError, match="gradcampp"):       # the reference has no audio Grad-CAM++
        EvalAudioBaselines("gradcampp", C.make_model())
    with pytest.raises(ValueError, match="layer="):
        EvalAudioBaselines("gradcam", testmodels.TinyAudio())
    with pytest.raises(ValueError, match="tie_order"):
        EvalAudioBaselines("saliency", C.make_model(), tie_order="random")
    with pytest.raises(RuntimeError):
        EvalAudioBaselines("saliency", C.make_model())       # a CPU model: the kernels run on the GPU only


# ------------------------------------------------------------------------------ restatement vs goldens
def _methods():
    return [(name, method) for name, case in C.CASES.items() for method in case["methods"]]


@pytest.mark.parametrize("name,method", _methods())
def test_restatement_explanations(name, method):
    case = C.CASES[name]
    x, y = C.make_inputs(case)
    got = A.compute_explanations(C.make_model(), method, x, y, C.cfg_of(case))
    ref = C.golden(name, method, "expl")
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    d = _distance(got, ref, method)
    print("%s %s: explanation distance %.3e" % (name, method, d))
    assert d <= BAR


@pytest.mark.parametrize("name,method", [(n, m) for n, m in _methods() if C.CASES[n]["methods"][m]])
def test_restatement_curves(name, method):
    """Run on the GOLDEN explanations, so that the ranking is the reference's: curves, scores, FF within
    1e-4, fidelity lists equal, and the masked rows equal to the C-ABI reference bit for bit."""
    case = C.CASES[name]
    x, y = C.make_inputs(case)
    model, cfg = C.make_model(), C.cfg_of(case)
    expl = C.golden(name, method, "expl")
    source = A.source_melspec(x, cfg).squeeze(1).numpy()
    P = source[0].size
    worst = 0.0
    for mode in C.MODES:
        for n_iter in case["methods"][method]:
            keep = []
            scores, curves, _ = A.evaluate_auc(model, expl, x, y, mode, n_iter, cfg, keep=keep)
            assert scores[0].dtype == np.float32 and curves[0].dtype == np.float32
            worst = max(worst, np.abs(np.array(curves) - C.golden(name, method, "%s_n%d_curves" % (mode, n_iter))).max(),
                        np.abs(np.array(scores) - C.golden(name, method, "%s_n%d_scores" % (mode, n_iter))).max())
            rank = np.stack([A.rank_of(A.descending_order(e)) for e in expl])
            rows = R1.rank_mask_rows_ref(source.reshape(C.N_CLIPS, P), rank, n_iter, int(P / n_iter), mode == "deletion")
            R1.assert_bits(np.stack(keep).reshape(rows.shape), rows, "%s n_iter %d masked rows" % (mode, n_iter))
    ff = A.faithfulness_of_spectra(model, expl, x, y, cfg)
    worst = max(worst, np.abs(np.array(ff) - C.golden(name, method, "ff")).max())
    print("%s %s: worst curve / score / FF distance %.3e" % (name, method, worst))
    assert worst <= BAR
    assert A.input_fidelity(model, expl, x, y, cfg) == C.golden(name, method, "fid").tolist()


def test_stable_sort_equals_numpy_without_ties():
    case = C.CASES["k4096"]
    expl = C.golden("k4096", "saliency", "expl")
    for e in expl:
        assert not C.straddling_ties(e, 7)
        if np.unique(e).size == e.size:
            assert np.array_equal(A.descending_order(e, "stable"), A.descending_order(e, "numpy"))
    x, y = C.make_inputs(case)
    a = A.evaluate_auc(C.make_model(), expl, x, y, "insertion", 7, C.cfg_of(case), sort="stable")[1]
    assert np.abs(np.array(a) - C.golden("k4096", "saliency", "insertion_n7_curves")).max() <= BAR


def test_nan_explanation_ranks_as_a_permutation():
    e = np.full((5, 7), np.nan, dtype=np.float32)
    for sort in ("numpy", "stable"):
        assert sorted(A.descending_order(e, sort).tolist()) == list(range(35))
