"""The numpy restatement of the pixel-domain baselines (tests/baselines_ref.py) against the reference's
own outputs (tests/golden/imgbase_goldens.npz, made by tests/golden/make_imgbase_goldens.py), on the CPU.

The restatement is what the GPU tests compare the device against, so it is pinned here first: image
bytes and model inputs exactly, curves and scores to 1e-4 (the float32 model evaluated in other batch
sizes), the CAMs within D_CAM (float64 sums against the reference's float32 channel loop).
"""
import random

import numpy as np
import pytest
import torch

from tests import baselines_ref as R
from tests.analyzer_ref import assert_bits
from tests.golden import imgbase_cases as C
from tests.helpers import npz


def G():
    return npz(C.GOLDENS)


def test_new_symbols_are_exported():
    import wam_amd
    import wam_amd.baselines as B
    from wam_amd.evaluation import EvalImageBaselines
    assert EvalImageBaselines is B.EvalImageBaselines is wam_amd.EvalImageBaselines
    for name in ("GradCAM", "GradCAMPlusPlus", "SmoothGrad", "Saliency", "IntegratedGradients"):
        assert getattr(wam_amd, name) is getattr(B, name)
    for name in ("wam_rank_mask_pixels", "wam_rank_mask_pixels_ws_bytes", "wam_cell_mask_pixels", "wam_cam_maps",
                 "wam_channel_mean"):
        assert hasattr(wam_amd._lib.lib, name)
    assert wam_amd._lib.lib.wam_rank_mask_pixels_ws_bytes(3, 7) == 8 * 3 * (8 + 32 * 9)   # the header's formula


def test_unsupported_and_unknown_methods_raise_at_construction():
    from wam_amd.baselines import EvalImageBaselines
    for name, package in (("guided_backprop", "captum"), ("layercam", "grad-cam"), ("lrp", "zennit"), ("srd", "SRD")):
        with pytest.raises(NotImplementedError, match=package):
            EvalImageBaselines(name, None)
    with pytest.raises(ValueError, match="unknown method"):
        EvalImageBaselines("gradcam++", None)
    from wam_amd.baselines import IntegratedGradients
    with pytest.raises(ValueError, match="riemann_trapezoid"):
        IntegratedGradients._prepare(None, None, None, "gausslegendre")


def test_host_argument_checks_need_no_device():
    from wam_amd._lib import lib
    assert lib.wam_rank_mask_pixels(1, 3, 16, None, None, 4, 4, 0, None, None, None, None, None, None, None) == 1
    assert lib.wam_cell_mask_pixels(5, 16, None, 1, 4, None, None, None, None, None, None, None, None) == 1
    assert lib.wam_cam_maps(1, 0, 2, 2, None, None, 0, 4, 4, None, None) == 1
    assert lib.wam_channel_mean(1, 3, 4, None, None, 0, None, None, None) == 1
    assert lib.wam_rank_mask_pixels_ws_bytes(-1, 4) < 0


@pytest.mark.parametrize("name", sorted(C.IMAGE_CASES))
@pytest.mark.parametrize("mode", C.MODES)
def test_image_bytes_reproduce_the_reference(name, mode):
    """Both forms: the line-by-line restatement (float64 masks, HWC) and the C-ABI reference (the rank
    rule of include/wam_hip.h on planar float32) give the reference's bytes."""
    img, expl, n_iter, rows = C.image_case(name)
    want = G()["img_%s_%s" % (name, mode)]
    ims = R.generate_images_baseline(img, expl, n_iter, mode)
    got = [ims[m] for m in rows]
    H, W = expl.shape
    order = np.argsort(expl, axis=None)[::-1]
    rank = np.empty(H * W, dtype=np.int32)
    rank[order] = np.arange(H * W)
    planar = np.moveaxis(img, 2, 0).reshape(1, 3, H * W)
    _, u8, _ = R.rank_mask_pixels_ref(planar, rank[None], n_iter, int(H * W / n_iter), mode == "deletion")
    abi = [np.moveaxis(u8[m].reshape(3, H, W), 0, 2) for m in rows]
    if name in C.DIGESTED:
        got, abi = [C.digest(a) for a in got], [C.digest(a) for a in abi]
    assert_bits(np.stack(got), want, "restatement")
    assert_bits(np.stack(abi), want, "C-ABI reference")


def test_cell_reference_equals_the_float64_mask_product():
    """v = grid * img in float32 is the reference's float64 mask product rounded to float32."""
    from wam_amd.evaluation import zoom_cell_map
    from scipy.ndimage import zoom
    rs = np.random.RandomState(3)
    img = rs.uniform(size=(64, 64, 3)).astype(np.float32)
    grid = np.ones((4, 8, 8))
    grid[:, :5] = rs.uniform(size=(4, 5, 8)).astype(np.float32)
    want = R.reconstruct_images_baseline(img, zoom(grid, (1, 8, 8), order=0))
    cell = zoom_cell_map(8, (64, 64)).reshape(-1)
    _, u8, _ = R.cell_mask_pixels_ref(np.moveaxis(img, 2, 0).reshape(3, -1), grid.reshape(4, -1), cell)
    for m in range(4):
        assert_bits(np.moveaxis(u8[m].reshape(3, 64, 64), 0, 2), want[m], "mask %d" % m)


def test_cams_within_d_cam(capsys):
    worst = 0.0
    for size in C.CAM_SIZES:
        x, y = C.cam_inputs(size)
        for layer in C.CAM_LAYERS:
            for name, pp in (("gradcam", False), ("gradcampp", True)):
                model = C.make_model()
                got = R.gradcam_ref(model, getattr(model, layer), x, y, pp)
                d = R.cam_distance(got, G()["cam_%s_%s_%d" % (name, layer, size)])
                worst = max(worst, d)
    with capsys.disabled():
        print("\nD_CAM measured: %.3e (constant %.1e)" % (worst, R.D_CAM))
    assert worst <= R.D_CAM
    for size in C.CAM_SIZES:  # the all-NaN map is part of the cases
        assert sum(np.isnan(m).all() for m in G()["cam_gradcam_conv2_%d" % size]) == 1


@pytest.mark.parametrize("name", sorted(C.CLASS_CASES))
@pytest.mark.parametrize("mode", C.MODES)
def test_class_curves_and_inputs(name, mode):
    case = C.CLASS_CASES[name]
    x, y, expl = C.class_inputs(case)
    seen = []
    scores, curves = R.evaluate_auc(C.make_model(), expl, x, y, mode, n_iter=case["n_iter"], seen=seen)
    g = G()
    assert np.abs(np.array(scores) - g["%s_%s_scores" % (name, mode)]).max() < 1e-4
    assert np.abs(np.array(curves) - g["%s_%s_curves" % (name, mode)]).max() < 1e-4
    got = np.stack([C.digest(seen[0][r]) for r in case["rows"]])
    assert_bits(got, g["%s_%s_inputs" % (name, mode)], "model inputs of image 0")


def test_mu_fidelity():
    case = C.MU_CASE
    x, y, expl = C.class_inputs(case)
    trace = []
    random.seed(case["pyseed"])
    mu = R.mu_fidelity(C.make_model(), expl, x, y, grid_size=case["grid_size"], sample_size=case["sample_size"],
                       subset_size=case["subset_size"], batch_size=case["batch_size"], trace=trace)
    g = G()
    for i, (bmask, ys, preds, attrs) in enumerate(trace):
        assert_bits(bmask, g["mu_bmask"][i], "baseline mask")
        assert np.abs(preds - g["mu_preds"][i]).max() < 1e-4
        assert np.abs(attrs - g["mu_attrs"][i]).max() <= 1e-6 * np.abs(g["mu_attrs"][i]).max()
    assert np.abs(np.array(mu) - g["mu_value"]).max() < 0.05


def test_saliency_end_to_end():
    case = C.SAL_CASE
    x, y, _ = C.class_inputs(case)
    g = G()
    expl = R.saliency_ref(C.make_model(), x, y)
    assert expl.dtype == np.float32
    assert np.abs(expl - g["sal_expl"]).max() <= 1e-6 * np.abs(g["sal_expl"]).max()
    for mode in C.MODES:
        scores, curves = R.evaluate_auc(C.make_model(), g["sal_expl"], x, y, mode, n_iter=case["n_iter"])
        assert np.abs(np.array(scores) - g["sal_%s_scores" % mode]).max() < 1e-4
        assert np.abs(np.array(curves) - g["sal_%s_curves" % mode]).max() < 1e-4


def test_channel_mean_reference_is_numpys_mean():
    rs = np.random.RandomState(9)
    g = rs.standard_normal((2, 3, 5, 7)).astype(np.float32)
    want = np.mean(np.transpose(g, (0, 2, 3, 1)), axis=-1)
    assert_bits(R.channel_mean_ref(g.reshape(2, 3, -1)).reshape(2, 5, 7), want, "channel mean")


def test_integrated_gradients_completeness():
    """The restated attribution sums to f(x) - f(0) up to the trapezoid's error (captum's delta)."""
    model = C.make_model()
    x = torch.tensor(np.random.RandomState(4).uniform(size=(2, 3, 32, 32)).astype(np.float32))
    y = [1, 3]
    attr = R.integrated_gradients_ref(model, x, y)
    with torch.no_grad():
        out = model(torch.cat([x, torch.zeros_like(x)])).numpy()
    want = np.array([out[i, y[i]] - out[2 + i, y[i]] for i in range(2)])
    assert np.abs(attr.reshape(2, -1).sum(1) - want).max() < 1e-3 * np.abs(want).max()
