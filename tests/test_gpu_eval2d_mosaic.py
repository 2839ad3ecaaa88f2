"""Eval2DWAM(mask_layout="mosaic") on the device against the float64 restatement of tests/eval2d_mosaic_ref.py
fed the evaluator's own grad_wams, its tie to the pinned "pywt" path on Haar, the held coefficients of a
non-Haar bank, and the behaviour of the default layout that must not move.

Bars: R.BAR = 1e-4 absolute on class probabilities and scores (the bar of
tests/test_gpu_eval.py for curves); 0.05 on mu-fidelity, a rank correlation over sample_size values
(tests/test_gpu_eval.py); bits where two device paths must coincide.
Measured on one MI355X: worst |p(device) - p(restatement)| 5.6e-6, worst score error 1.6e-5; mu-fidelity
equal to the restatement's in every printed digit; eval_batch moves a probability by 6.0e-8 at most.
"""
import random

import numpy as np
import pytest
import torch

import testmodels
from tests import eval2d_mosaic_ref as R

pytestmark = pytest.mark.gpu
CASES = {"haar_J2": ("haar", 2, 1), "db2_J2": ("db2", 2, 1), "db6_J1": ("db6", 1, 0)}    # wavelet, J, route
Y = [1, 3, 7]
N_ITER = 8
S = 32
_EVALS = {}
WORST = {"dp": 0.0, "dscore": 0.0}


def images():
    return torch.rand(3, 3, S, S, generator=torch.Generator().manual_seed(S))


def make_eval(name, **kw):
    from wam_amd import Eval2DWAM
    wavelet, J, route = CASES[name]
    kw.setdefault("mask_layout", "mosaic")
    ev = Eval2DWAM(testmodels.TinySmooth2D().cuda(), wavelet=wavelet, J=J, n_samples=2, frame="native", **kw)
    ev.ranked_route = route
    return ev


def shared_eval(name):
    """One evaluator per case; its grad_wams are computed by the first test that needs them."""
    if name not in _EVALS:
        ev = make_eval(name)
        ev.grad_wams = ev.smooted_grad_wam(images(), Y)
        _EVALS[name] = ev
    return _EVALS[name]


def eval_plan(name):
    from wam_amd.plan import get_plan
    wavelet, J, _ = CASES[name]
    return get_plan(2, (S, S), J, wavelet, "symmetric", "cuda")


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    d = float(np.abs(got - want).max())
    print("[eval2d mosaic] %s: max |d| = %.3e" % (what, d))
    return d


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_class_against_the_restatement(name):
    wavelet, J, route = CASES[name]
    x = images()
    ev = shared_eval(name)
    plan = eval_plan(name)
    if route == 0:
        assert plan.ranked2_route() == 0                        # 12 taps: the expansion route by itself
    pos, shape, held = ev._mosaic_layout(plan)
    cell, ref_shape = R.coeff_cells(S, S, J, wavelet)
    assert shape == ref_shape == (S, S) and ev.grad_wams.shape == (3, S, S)
    assert held == int((cell == R.HELD).sum()) and (held > 0) == (wavelet != "haar")
    assert np.array_equal(pos.cpu().numpy(), np.where(cell == R.HELD, S * S, cell))
    model = testmodels.TinySmooth2D()
    for mode in ("insertion", "deletion"):
        scores = getattr(ev, mode)(x, Y, n_iter=N_ITER)
        curves = getattr(ev, mode + "_curves")
        want_scores, want_curves = R.evaluate_auc(model, ev.grad_wams, x, Y, mode, J, wavelet, N_ITER)
        assert np.array(curves).shape == (3, N_ITER + 1) and isinstance(scores, list)
        dp = close(curves, want_curves, "%s %s curves" % (name, mode))
        ds = close(scores, want_scores, "%s %s scores" % (name, mode))
        WORST["dp"], WORST["dscore"] = max(WORST["dp"], dp), max(WORST["dscore"], ds)
        assert dp <= R.BAR and ds <= R.BAR, (name, mode, dp, ds)


def test_mu_fidelity_against_the_restatement():
    name = "db2_J2"
    wavelet, J, _ = CASES[name]
    x = images()[:2]
    y = Y[:2]
    ev = make_eval(name, batch_size=16)
    ev.grad_wams = shared_eval(name).grad_wams[:2]
    random.seed(3)
    got = ev.mu_fidelity(x, y, grid_size=8, sample_size=16, subset_size=20)
    random.seed(3)
    want = R.mu_fidelity(testmodels.TinySmooth2D(), ev.grad_wams, x, y, J, wavelet, grid_size=8, sample_size=16,
                         subset_size=20, batch_size=16)
    print("[eval2d mosaic] mu-fidelity device %s restatement %s" % (got, want))
    assert len(got) == 2 and np.abs(np.array(got) - np.array(want)).max() < 0.05


def swap_h_v(w, J):
    """The mosaic with the horizontal (top-right) and vertical (bottom-left) blocks of every level
    exchanged: where pywt's coeffs_to_array keeps cV and cH."""
    out = w.copy()
    for i in range(J):
        e, s = S // 2 ** i, S // 2 ** (i + 1)
        out[:s, s:e] = w[s:e, :s]
        out[s:e, :s] = w[:s, s:e]
    return out


@pytest.mark.parametrize("deletion", [False, True])
def test_haar_mosaic_equals_the_pinned_layout_with_h_and_v_exchanged(deletion):
    name = "haar_J2"
    _, J, _ = CASES[name]
    rs = np.random.RandomState(11)
    w = rs.permutation(S * S).reshape(S, S).astype(np.float64) / 7.0
    assert np.unique(w).size == w.size                          # a tie would let the two rankings differ
    wx = swap_h_v(w, J)
    x = images()[:1]
    mos, pin = make_eval(name), make_eval(name, mask_layout="pywt")
    img = mos._images(x)[0]
    a = mos._ranked_inputs(img[None], w[None], N_ITER, deletion)
    b = pin._altered_inputs(img, pin._rank_masks(wx, N_ITER, deletion))
    assert a.shape == b.shape == (N_ITER + 1, 3, 224, 224) and same_bits(a, b)
    mos.ranked_route = 0
    assert same_bits(mos._ranked_inputs(img[None], w[None], N_ITER, deletion), b)
    mode = "deletion" if deletion else "insertion"
    mos.grad_wams, pin.grad_wams = w[None], wx[None]
    getattr(mos, mode)(x, Y[:1], n_iter=N_ITER), getattr(pin, mode)(x, Y[:1], n_iter=N_ITER)
    assert close(getattr(mos, mode + "_curves"), getattr(pin, mode + "_curves"), "haar mosaic vs pywt " + mode) <= R.BAR


@pytest.mark.parametrize("route", [0, 1])
def test_held_coefficients_db2(route):
    name = "db2_J2"
    ev = make_eval(name)
    ev.ranked_route = route
    plan = eval_plan(name)
    pos, shape, held = ev._mosaic_layout(plan)
    assert held > 0
    x = images()[:2]
    imgs = torch.stack(ev._images(x))
    wams = np.random.RandomState(5).standard_normal((2, S, S))
    coeffs = plan.wavedec(imgs.contiguous())
    exact = plan.waverec(coeffs, 6)[0].view(2, 3, S, S)
    only_held = coeffs.clone()
    keep = (pos == S * S).float()
    for b, view in enumerate(plan.split(only_held, 6)):
        view.mul_(keep[plan.band_offsets[b]:plan.band_offsets[b + 1]].view(plan.band_shapes[b]))
    held_rec = plan.waverec(only_held, 6)[0].view(2, 3, S, S)
    _, ins = ev._ranked_recs(imgs, wams, N_ITER, False)
    _, dele = ev._ranked_recs(imgs, wams, N_ITER, True)
    assert ins.shape == (2, N_ITER + 1, 3, S, S)
    assert same_bits(ins[:, 0], held_rec) and same_bits(dele[:, N_ITER], held_rec)
    assert same_bits(ins[:, N_ITER], exact) and same_bits(dele[:, 0], exact)
    assert not same_bits(held_rec, torch.zeros_like(held_rec))


def test_default_layout_still_raises_for_db4_and_bad_layouts_raise():
    from wam_amd import Eval2DWAM
    model = testmodels.TinySmooth2D().cuda()
    ev = Eval2DWAM(model, wavelet="db4", J=3, n_samples=2, frame="native")
    assert ev.mask_layout == "pywt"
    ev.grad_wams = np.random.RandomState(0).standard_normal((1, S, S))
    with pytest.raises(ValueError, match="could not be broadcast"):
        ev.insertion(images()[:1], Y[:1], n_iter=N_ITER)
    with pytest.raises(ValueError, match="mask_layout"):
        Eval2DWAM(model, mask_layout="mosiac")
    mos = make_eval("db2_J2")
    mos.grad_wams = np.zeros((1, S + 2, S + 2))
    with pytest.raises(ValueError, match="could not be broadcast"):
        mos.insertion(images()[:1], Y[:1], n_iter=N_ITER)


@pytest.mark.parametrize("name", ["haar_J2", "db6_J1"])
def test_eval_batch_does_not_change_the_curves(name):
    """eval_batch = n_iter + 1 (one image per call and forward) and the default (all three in one)."""
    x = images()
    ev = shared_eval(name)
    one = make_eval(name, eval_batch=N_ITER + 1)
    one.grad_wams = ev.grad_wams
    for mode in ("insertion", "deletion"):
        getattr(one, mode)(x, Y, n_iter=N_ITER), getattr(ev, mode)(x, Y, n_iter=N_ITER)
        assert close(getattr(one, mode + "_curves"), getattr(ev, mode + "_curves"),
                     "eval_batch %s %s" % (name, mode)) <= R.BAR
