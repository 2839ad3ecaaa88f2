"""Eval3DWAM.mu_fidelity on the device against the float64 restatement of tests/eval3d_mu_ref.py, which is
fed the evaluator's own grad_wams and the device's baseline_index.

rho is not compared with the restatement's rho: on these inputs the restatement's smallest gap between
sorted probability drops is 2.4e-7 to 2.3e-5, the device's recorded error on a probability is 1.2e-7
(tests/test_gpu_eval3d.py), and one swap among 16 samples moves rho by about 3e-3. What is compared:

  baseline_probs, altered_probs   R.BAR = 1e-4 absolute, the project's bar on class probabilities
  baseline_index                  ref_pb[index] - ref_pb.min() <= 2 * R.BAR: within the bar on both sides of
                                  the restatement's own minimum (its own argmin meets it with 0)
  sums                            evalkern_ref.assert_sum_bound: (len + 1) * 2^-53 * S_m
  mu                              == spearmanr(base - altered_probs, sums).statistic from the device's own
                                  details, to 1e-12, the reference's sums being free of near-ties (1e-9
                                  relative)

Measured on one MI355X (printed when the module finishes): worst |p(device) - p(restatement)| 1.19e-7,
worst baseline-index excess 0.0 (the device's index was the restatement's own argmin at all 12 volumes), worst sums
error / bound 0.0039.
"""
import random

import numpy as np
import pytest
import torch
from scipy.stats import spearmanr

from tests import eval3d_mu_ref as R
from tests import evalkern_ref as K

pytestmark = pytest.mark.gpu
# name -> (S, J, grid, sample_size, subset_size); J <= 2: the fused route, J = 3: the expansion route
CASES = {"S8_J1_g4": (8, 1, 4, 16, 13), "S8_J2_g4": (8, 2, 4, 16, 13), "S8_J2_g3": (8, 2, 3, 12, 6),
         "S16_J3_g4": (16, 3, 4, 16, 13)}
Y = [1, 3, 7]
WORST = {"dp": 0.0, "dindex": 0.0, "dsum": 0.0}
_EVALS = {}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()
    print("[eval3d mu] worst |p(device) - p(restatement)| %.3e (bar %.1e), worst baseline-index excess %.3e (bar "
          "%.1e), worst sums error / bound %.3g" % (WORST["dp"], R.BAR, WORST["dindex"], 2 * R.BAR, WORST["dsum"]))


def volumes(S):
    return torch.rand(3, 1, S, S, S, generator=torch.Generator().manual_seed(S))


def make_eval(name, **kw):
    import testmodels
    from wam_amd.evaluation import Eval3DWAM
    return Eval3DWAM(testmodels.TinyVoxel().cuda(), wavelet="haar", J=CASES[name][1], n_samples=2, **kw)


def run(ev, name):
    S, J, g, sample_size, subset_size = CASES[name]
    return ev.mu_fidelity(volumes(S), Y, grid_size=g, sample_size=sample_size, subset_size=subset_size)


def shared(name):
    """One evaluator per case (its grad_wams computed by its first call, counted), its scores, details and
    the restatement fed the device's grad_wams and baseline_index."""
    if name not in _EVALS:
        import testmodels
        S, J, g, sample_size, subset_size = CASES[name]
        ev = make_eval(name)
        calls = []
        inner = ev.gradwam
        ev.gradwam = lambda *a: calls.append(1) or inner(*a)
        mu = run(ev, name)
        details = ev.mu_details
        ref = R.mu_fidelity(testmodels.TinyVoxel(), volumes(S).numpy(), Y, ev.grad_wams, J, g, sample_size, subset_size,
                            baseline_index=[d["baseline_index"] for d in details])
        _EVALS[name] = (ev, calls, mu, details, ref)
    return _EVALS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_details_against_the_restatement(L, name):
    from wam_amd.plan import get_plan
    S, J, g, sample_size, subset_size = CASES[name]
    ev, calls, mu, details, ref = shared(name)
    plan = get_plan(3, (S, S, S), J, "haar", "symmetric", "cuda")
    assert plan.cells_route in (0, 1) and (J <= 2 or plan.cells_route == 0)         # J = 3: the expansion route
    assert isinstance(mu, list) and len(mu) == 3 and len(details) == 3 and ev.grad_wams.shape == (3, S, S, S)
    for i, (d, r) in enumerate(zip(details, ref)):
        for key in ("baseline_probs", "altered_probs", "sums"):
            assert np.asarray(d[key]).shape == (sample_size,) and np.isfinite(d[key]).all(), (name, i, key)
        dp = max(float(np.abs(d["baseline_probs"] - r["baseline_probs"]).max()),
                 float(np.abs(d["altered_probs"] - r["altered_probs"]).max()))
        b = d["baseline_index"]
        dindex = float(r["baseline_probs"][b] - r["baseline_probs"].min())
        print("[eval3d mu] %s volume %d: max |dp| = %.3e, baseline index %d excess %.3e, mu %.6f (restatement %.6f)"
              % (name, i, dp, b, dindex, mu[i], r["mu"]))
        WORST["dp"], WORST["dindex"] = max(WORST["dp"], dp), max(WORST["dindex"], dindex)
        assert dp <= R.BAR, (name, i, dp)
        assert 0 <= b < sample_size and dindex <= 2 * R.BAR, (name, i, b, dindex)
        WORST["dsum"] = max(WORST["dsum"], K.assert_sum_bound(d["sums"], r["sums"], r["sum_mags"], S ** 3,
                                                              "mu_sums %s volume %d" % (name, i)))
        # a condition on the reference alone: no two of its sums within 1e-9 relative of each other
        rs = np.sort(r["sums"])
        assert (np.diff(rs) > 1e-9 * np.abs(rs[1:])).all(), (name, i)
        want = spearmanr(np.float64(d["base_prob"]) - np.asarray(d["altered_probs"], dtype=np.float64),
                         d["sums"]).statistic
        assert abs(mu[i] - float(want)) <= 1e-12, (name, i, mu[i], want)
        assert abs(float(d["base_prob"]) - float(r["base_prob"])) <= R.BAR


def test_grad_wams_once_and_fresh_draws(L):
    ev, calls, mu, details, _ = shared("S8_J2_g4")
    again = run(ev, "S8_J2_g4")
    assert len(calls) == 1                                       # the second call does not recompute grad_wams
    assert again == mu                                           # fresh generators: the same draws, the same bits
    for a, b in zip(ev.mu_details, details):
        assert a["baseline_index"] == b["baseline_index"] and np.array_equal(a["altered_probs"], b["altered_probs"])


def test_global_random_state_is_left_alone(L):
    ev = shared("S8_J1_g4")[0]
    random.seed(5)
    np.random.seed(5)
    st, nst = random.getstate(), np.random.get_state()
    run(ev, "S8_J1_g4")
    now = np.random.get_state()
    assert random.getstate() == st and now[0] == nst[0] and np.array_equal(now[1], nst[1]) and now[2:] == nst[2:]


def test_compute_baseline_state_returns_the_source_mask(L):
    name = "S8_J2_g4"
    S, J, g, sample_size, subset_size = CASES[name]
    ev, _, _, details, ref = shared(name)
    x = volumes(S)
    # volume 0's candidates are the first draw of RandomState(random_seed): the default source
    got = ev.compute_baseline_state(x[0], Y[0], grid_size=g, sample_size=sample_size)
    assert got.shape == (g, g, g) and got.dtype == np.float32
    assert np.array_equal(got, ref[0]["source"][details[0]["baseline_index"]])
    # any volume with its own candidates handed over
    got = ev.compute_baseline_state(x[2, 0], Y[2], grid_size=g, source=ref[2]["source"])
    assert np.array_equal(got, ref[2]["source"][details[2]["baseline_index"]])


@pytest.mark.parametrize("name", ["S8_J2_g4", "S16_J3_g4"])
def test_eval_batch_does_not_change_the_details(L, name):
    """eval_batch = the default (all three volumes in one call), sample_size (one volume per call) and
    sample_size // 2 (two forwards per volume)."""
    S, J, g, sample_size, subset_size = CASES[name]
    ev, _, mu, details, _ = shared(name)
    for eb in (sample_size, sample_size // 2):
        one = make_eval(name, eval_batch=eb)
        one.grad_wams = ev.grad_wams
        run(one, name)
        for a, b in zip(one.mu_details, details):
            assert a["baseline_index"] == b["baseline_index"]
            assert np.abs(a["baseline_probs"] - b["baseline_probs"]).max() <= R.BAR
            assert np.abs(a["altered_probs"] - b["altered_probs"]).max() <= R.BAR
            K.assert_bits(a["sums"], b["sums"], "sums do not depend on eval_batch")


def test_cells_routes_give_identical_altered_probs(L):
    """The kernels are bit-identical and the model batch is the same."""
    name = "S8_J2_g4"
    ev = shared(name)[0]
    got = []
    for route in (0, 1):
        one = make_eval(name)
        one.grad_wams = ev.grad_wams
        one.cells_route = route
        got.append((run(one, name), one.mu_details))
    assert got[0][0] == got[1][0]
    for a, b in zip(got[0][1], got[1][1]):
        assert a["baseline_index"] == b["baseline_index"]
        assert np.array_equal(a["altered_probs"], b["altered_probs"]) and np.array_equal(a["baseline_probs"], b["baseline_probs"])
    # route 1 forced where the fused kernel does not apply is an error, not a fallback
    from wam_amd._lib import WamError
    bad = make_eval("S16_J3_g4")
    bad.grad_wams = shared("S16_J3_g4")[0].grad_wams
    bad.cells_route = 1
    with pytest.raises(WamError):
        run(bad, "S16_J3_g4")


def test_bad_arguments_raise(L):
    ev = make_eval("S8_J2_g4")
    with pytest.raises(ValueError, match="labels"):
        ev.mu_fidelity(volumes(8), None)
    ev.grad_wams = np.zeros((1, 8, 8, 16), np.float32)
    with pytest.raises(ValueError, match="cubic"):
        ev.mu_fidelity(torch.rand(1, 1, 8, 8, 16), [0], grid_size=4, sample_size=4)
    ev.grad_wams = np.zeros((1, 10, 10, 10), np.float32)
    with pytest.raises(ValueError, match="bijection onto the coefficients"):
        ev.mu_fidelity(torch.rand(1, 1, 10, 10, 10), [0], grid_size=4, sample_size=4)
    ev.grad_wams = np.zeros((1, 8, 8, 8), np.float32)
    with pytest.raises(ValueError, match="grid_size"):
        ev.mu_fidelity(torch.rand(1, 1, 8, 8, 8), [0], grid_size=9, sample_size=4)
    # a constant attribution: constant sums, rho is NaN
    mu = ev.mu_fidelity(torch.rand(1, 1, 8, 8, 8), [0], grid_size=4, sample_size=4, subset_size=13)
    assert len(mu) == 1 and np.isnan(mu[0])
