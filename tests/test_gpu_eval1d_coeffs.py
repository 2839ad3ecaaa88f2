"""Eval1DWAM(mask_layout="coeffs") on the device: every coefficient ranked by its own gradient, any
wavelet. The reference is the plain-numpy restatement of tests/eval1d_ref.py run with
Rules(offsets="running") -- the bands' own running offsets, which is this layout -- on inputs whose
properties were checked on the CPU beforehand (no tie straddles a threshold at n_iter 4 or 7, the
restatement's float32-synthesis spread is at most 3.7e-8, the top two logits behind every
input-fidelity arg-max are at least 0.078 apart): rs = RandomState(7), x = rs.standard_normal((2, W)),
then per band rs.standard_normal((2, n_i)), float32, y = [1, 4].

The bar is R.BAR = 1e-4 on class probabilities, scores and faithfulness of spectra, as in
tests/test_gpu_eval1d.py. The db6 and db2 cases cannot run without the layout: the keyword is a
TypeError there, and without it every non-Haar wavelet is the reference's broadcast ValueError.
"""
import numpy as np
import pytest
import torch

from tests import eval1d_ref as R
from tests.golden.eval1d_cases import CASES, COMMON, GOLDENS as G, golden_grad_wams, make_inputs, make_model
from tests.helpers import npz

pytestmark = pytest.mark.gpu
N_FFT = 256
Y = [1, 4]
# wavelet, J, W
GEOMS = {"db6_4096": ("db6", 3, 4096), "db2_9001": ("db2", 2, 9001), "sym4_8300": ("sym4", 4, 8300)}
_INPUTS, _REF = {}, {}


def cfg(name):
    wavelet, J, _ = GEOMS[name]
    return dict(wavelet=wavelet, J=J, n_fft=N_FFT, sample_rate=COMMON["sample_rate"], n_mels=COMMON["n_mels"])


def inputs(name):
    """(x float32 [2, W], grad_wams): made once per geometry and never changed."""
    if name not in _INPUTS:
        from wam_amd.plan import get_plan
        wavelet, J, W = GEOMS[name]
        plan = get_plan(1, (W,), J, wavelet, "reflect", "cuda")
        rs = np.random.RandomState(7)
        x = rs.standard_normal((2, W)).astype(np.float32)
        grads = [rs.standard_normal((2, s[0])).astype(np.float32) for s in plan.band_shapes]
        _INPUTS[name] = (x, (np.zeros((2, 3, COMMON["n_mels"]), np.float32), grads))
    return _INPUTS[name]


def restated(name, mode, n_iter, silent):
    """The restatement's (scores, curves, raw logits), computed once per key and shared."""
    key = (name, mode, n_iter, silent)
    if key not in _REF:
        x, gw = inputs(name)
        _REF[key] = R.evaluate_auc(make_model(), x, Y, gw, mode, "wavelet", n_iter, cfg(name),
                                   R.Rules(offsets="running", silent=silent))
    return _REF[key]


def make_eval(name, inject=True, **kw):
    from wam_amd.evaluation import Eval1DWAM
    wavelet, J, _ = GEOMS[name]
    ev = Eval1DWAM(make_model().cuda(), 128, wavelet, J, "smooth", "reflect", None, False, COMMON["n_mels"], N_FFT,
                   COMMON["sample_rate"], COMMON["n_samples"], mask_layout="coeffs", **kw)
    if inject:
        ev.grad_wams = inputs(name)[1]
    return ev


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern %s vs %s" % (what, got, want)
    d = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
    print("[eval1d_coeffs] %s: max |d| = %.3e" % (what, d))
    return d


@pytest.mark.parametrize("silent", ["nan", "zero"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_class_against_the_restatement(name, silent):
    """Curves, scores and faithfulness of spectra within R.BAR of the restatement with running
    offsets, the NaN pattern equal (one NaN row per clip under 'nan', none under 'zero'), the
    input-fidelity lists equal."""
    x, _ = inputs(name)
    ev = make_eval(name, tie_order="numpy", silent=silent)
    xt = torch.tensor(x)
    for mode in ("insertion", "deletion"):
        for n_iter in (4, 7):
            scores = getattr(ev, mode)(xt, Y, "wavelet", n_iter)
            curves = np.array(getattr(ev, mode + "_curves"))
            want_scores, want_curves, _ = restated(name, mode, n_iter, silent)
            what = "%s %s n%d silent=%s" % (name, mode, n_iter, silent)
            assert close(curves, want_curves, what + " curves") <= R.BAR
            assert close(scores, want_scores, what + " scores") <= R.BAR
            nan_rows = np.isnan(curves).sum(axis=1).tolist()
            assert nan_rows == ([1, 1] if silent == "nan" else [0, 0])
            assert np.isfinite(scores).all() == (silent == "zero")
    _, c2, _ = restated(name, "deletion", 2, silent)
    c2 = np.array(c2)
    assert close(ev.faithfulness_of_spectra(xt, Y, "wavelet"), (c2[:, 0] - c2[:, 1]).tolist(), name + " ff") <= R.BAR
    _, _, raw = restated(name, "insertion", 2, silent)
    logits = np.sort(np.array(raw)[:, 1:, :], axis=2)
    assert (logits[..., -1] - logits[..., -2]).min() >= 0.03
    assert ev.input_fidelity(xt, Y, "wavelet") == np.argmax(np.array(raw)[:, 1:, :], axis=2).tolist()
    assert ev.grad_wams is inputs(name)[1]        # the injected maps were used, not recomputed


@pytest.mark.parametrize("mode", ["insertion", "deletion"])
def test_haar_dyadic_equals_the_default_layout(mode):
    """Golden case k4096 (Haar, dyadic length: the reference's slices are the bands' own): 'coeffs'
    gives the default layout's curves exactly, and both are within R.BAR of the reference's goldens."""
    from wam_amd.evaluation import Eval1DWAM
    case = CASES["k4096"]
    x, y = make_inputs(case)
    d = npz(G)
    evs = []
    for layout in ("reference", "coeffs"):
        ev = Eval1DWAM(make_model().cuda(), 128, case["wavelet"], case["J"], "smooth", "reflect", None, False,
                       COMMON["n_mels"], case["n_fft"], COMMON["sample_rate"], COMMON["n_samples"], tie_order="numpy",
                       mask_layout=layout)
        ev.grad_wams = golden_grad_wams("k4096")
        evs.append(ev)
    for n_iter in (4, 7):
        got = []
        for ev in evs:
            getattr(ev, mode)(x, y, "wavelet", n_iter)
            got.append(np.array(getattr(ev, mode + "_curves")))
        assert np.array_equal(got[0], got[1], equal_nan=True), n_iter
        assert close(got[1], d["k4096_wavelet_%s_n%d_curves" % (mode, n_iter)], "k4096 %s n%d" % (mode, n_iter)) <= R.BAR


def test_forced_routes_give_equal_curves():
    """ranked_route 0 and 1 on db6: the two routes are bit-identical, so the curves are equal."""
    name = "db6_4096"
    xt = torch.tensor(inputs(name)[0])
    curves = []
    for route in (0, 1):
        ev = make_eval(name, tie_order="numpy", silent="zero")
        ev.ranked_route = route
        ev.deletion(xt, Y, "wavelet", 7)
        curves.append(np.array(ev.deletion_curves))
    assert np.array_equal(curves[0], curves[1])


def test_eval_batch_does_not_change_the_curves():
    """eval_batch = n_iter + 1 (one clip per call) and 520 (both clips in one) on db2 at 9,001 samples."""
    name = "db2_9001"
    xt = torch.tensor(inputs(name)[0])
    one = make_eval(name, tie_order="numpy", silent="zero", eval_batch=8)
    both = make_eval(name, tie_order="numpy", silent="zero", eval_batch=520)
    one.insertion(xt, Y, "wavelet", 7), both.insertion(xt, Y, "wavelet", 7)
    assert close(one.insertion_curves, both.insertion_curves, "eval_batch") <= R.BAR
    assert close(one.insertion_curves, restated(name, "insertion", 7, "zero")[1], "eval_batch 8 vs restatement") <= R.BAR


def test_errors():
    from wam_amd.evaluation import Eval1DWAM
    with pytest.raises(ValueError, match="mask_layout must be 'reference' or 'coeffs', got 'mosaic'"):
        Eval1DWAM(make_model().cuda(), wavelet="db6", J=3, mask_layout="mosaic")
    name = "db6_4096"
    x, (mel, grads) = inputs(name)
    ev = make_eval(name, inject=False)
    ev.grad_wams = (mel, [g[:, :-1] if i == 1 else g for i, g in enumerate(grads)])     # band 1 one short
    with pytest.raises(ValueError, match=r"the explainer's bands \[.*\] are not the evaluation plan's \[.*\]"):
        ev.insertion(torch.tensor(x), Y, "wavelet", 4)


def test_end_to_end_db6():
    """No injection: grad_wams computed once by the inner WaveletAttribution1D and cached; the curves are
    within the bar of the restatement fed those maps (tie_order='numpy': the same np.argsort)."""
    name = "db6_4096"
    x = inputs(name)[0]
    xt = torch.tensor(x)
    ev = make_eval(name, inject=False, tie_order="numpy", silent="zero")
    calls = []
    inner = ev.gradwam
    ev.gradwam = lambda *a: calls.append(1) or inner(*a)
    ev.insertion(xt, Y, "wavelet", 4)
    gw = ev.grad_wams
    ev.deletion(xt, Y, "wavelet", 4)
    assert len(calls) == 1 and ev.grad_wams is gw
    assert [np.asarray(b).shape[1] for b in gw[1]] == [g.shape[1] for g in inputs(name)[1][1]]
    model = make_model()
    rules = R.Rules(offsets="running", silent="zero")
    for mode, curves in (("insertion", ev.insertion_curves), ("deletion", ev.deletion_curves)):
        _, want, _ = R.evaluate_auc(model, x, Y, gw, mode, "wavelet", 4, cfg(name), rules)
        assert np.isfinite(np.array(want)).all()
        assert close(curves, want, "end to end db6 %s" % mode) <= R.BAR
