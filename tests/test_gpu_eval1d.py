"""Eval1DWAM on the device: the three kernels of wam_amd/csrc/evaluate1d.hip at the C ABI, bit for bit
against the numpy references of tests/eval1d_ref.py, and the class against the goldens made by the
reference's own Eval1DWAM (tests/golden/eval1d_goldens.npz).

The bar of the class tests is R.BAR = max(1e-4, 4 * d32) on class probabilities (absolute): 1e-4 is
the 2D evaluator's bar, d32 = 5.96e-8 the spread the float64 restatement shows when its synthesis
and normalisation run in float32 (tests/test_eval1d_ref.py measures it), so the bar is 1e-4.
Curves, scores and faithfulness of spectra are all held to that one bar. Measured on one MI355X over
all cases, targets, modes and n_iter: worst |p(device) - p(golden)| = 1.04e-7, worst score error
1.19e-7, worst faithfulness-of-spectra error 8.9e-8 (printed when the module finishes).
"""
import numpy as np
import pytest
import torch

from tests import eval1d_ref as R
from tests.golden.eval1d_cases import (CASES, GOLDENS as G, MODES, N_CLIPS, N_ITERS, TARGETS, cfg_of, ctor_kw,
                                       golden_grad_wams, make_inputs, make_model)
from tests.helpers import npz

pytestmark = pytest.mark.gpu
WORST = {"dp": 0.0, "dscore": 0.0, "dff": 0.0}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()
    print("[eval1d] worst |device - golden|: p %.3e, score %.3e, faithfulness of spectra %.3e (bar %.1e)"
          % (WORST["dp"], WORST["dscore"], WORST["dff"], R.BAR))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ranks(rng, sets, n):
    return np.stack([rng.permutation(n) for _ in range(sets)]).astype(np.int32)


# ------------------------------------------------------------------------------ kernels
COEFF_CASES = {
    # bands 10, 10, 19 (offsets 0, 10, 20: the scalar path), band 1 ends in the pad column
    "haar_37_J2": (37, 2, 5),
    # bands 501, 501, 1001, 2001 (scalar path), more than one block per band
    "haar_4002_J3": (4002, 3, 5),
    # bands 512, 512, 1024, 2048 (16-byte path); n_comp * n_iter = 4095 < 4096: the forced last mask
    "haar_4096_J3_n7": (4096, 3, 7),
}


@pytest.mark.parametrize("deletion", [0, 1])
@pytest.mark.parametrize("name", list(COEFF_CASES))
def test_rank_mask_coeffs(L, name, deletion):
    """wam_rank_mask_coeffs vs rank_mask_coeffs_ref, 3 sets: bit-equal (signed zeros of dropped
    negative values included). The slot maps are Eval1DWAM's own; the 4096 case adds one -1 and one
    out-of-range slot on the 16-byte path, and checks that the 16-byte path is the one taken."""
    from wam_amd.evaluation import coeff_slot_map
    from wam_amd.plan import get_plan
    length, J, n_iter = COEFF_CASES[name]
    sets = 3
    p = get_plan(1, (length,), J, "haar", "reflect", "cuda")
    off = list(p.band_offsets)
    K = off[-1]
    pos = coeff_slot_map(length, J, [s[0] for s in p.band_shapes])
    if name == "haar_37_J2":
        assert np.diff(off).tolist() == [10, 10, 19] and (pos == -1).sum() == 1 and pos[19] == -1
    if name == "haar_4002_J3":
        assert np.diff(off).tolist() == [501, 501, 1001, 2001] and (pos == -1).sum() == 1
    if name == "haar_4096_J3_n7":
        assert all(o % 4 == 0 for o in off) and int(K / n_iter) * n_iter < K
        pos = pos.copy()
        pos[700], pos[3001] = -1, K + 5
    rng = np.random.RandomState(length + deletion)
    coeffs = rng.standard_normal(sets * K).astype(np.float32)
    rank = ranks(rng, sets, K)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    out = torch.full((sets * (n_iter + 1) * K,), 7.0, device="cuda")
    assert dc.data_ptr() % 16 == 0 and dp.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    L.check(L.lib.wam_rank_mask_coeffs(p.handle, sets, L.ptr(dc), L.ptr(dr), K, L.ptr(dp), n_iter, int(K / n_iter),
                                       deletion, L.ptr(out), L.stream_of(out.device)))
    ref = R.rank_mask_coeffs_ref(off, sets, coeffs, rank, pos, n_iter, int(K / n_iter), deletion)
    R.assert_bits(out.cpu().numpy(), ref, "rank_mask_coeffs %s del=%d" % (name, deletion))
    # the output is what wam_waverec reads: item (s, n_iter) under insertion is the unmasked set
    if not deletion and name != "haar_4096_J3_n7":
        rec = p.waverec(out, sets * (n_iter + 1))[0].view(sets, n_iter + 1, -1)
        full = p.waverec(dc, sets)[0]
        assert torch.equal(rec[:, n_iter], full)


@pytest.mark.parametrize("deletion", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1031])
def test_rank_mask_rows(L, n, deletion):
    """wam_rank_mask_rows vs rank_mask_rows_ref, 3 sets, n_iter = 5: bit-equal. 64: the 16-byte path;
    1: n_comp = 0, only the forced last mask selects."""
    sets, n_iter = 3, 5
    rng = np.random.RandomState(n + deletion)
    src = rng.standard_normal((sets, n)).astype(np.float32)
    rank = ranks(rng, sets, n)
    out = torch.full((sets, n_iter + 1, n), 7.0, device="cuda")
    ds, dr = dev(src), dev(rank)   # held in names: a temporary's memory would be reused by the next one
    L.check(L.lib.wam_rank_mask_rows(sets, n, L.ptr(ds), L.ptr(dr), n_iter, int(n / n_iter), deletion,
                                     L.ptr(out), L.stream_of(out.device)))
    R.assert_bits(out.cpu().numpy(), R.rank_mask_rows_ref(src, rank, n_iter, int(n / n_iter), deletion),
                  "rank_mask_rows n=%d del=%d" % (n, deletion))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099, 80000])
def test_peak_normalize(L, n, in_place):
    """wam_peak_normalize vs peak_normalize_ref: bit-equal (IEEE division). Rows: maximum first,
    maximum last, all negative (the signed maximum is negative: the signs flip), all zero (silent:
    NaN, or unchanged with zero_silent), non-positive with zeros (silent: -inf and NaN), random.
    Multiples of 4 take the 16-byte path, 80,000 the 1,024-thread workgroup."""
    rng = np.random.RandomState(n)
    x = rng.uniform(-1, 1, (7, n)).astype(np.float32)
    x[0, 0], x[1, -1] = 3.0, 2.5
    x[2] = -np.abs(x[2]) - 0.25
    x[3] = 0.0
    x[4] = -np.abs(x[4])
    x[4, n // 2] = 0.0
    for zero_silent in (0, 1):
        src = dev(x)
        out = src if in_place else torch.full_like(src, 7.0)
        silent = torch.full((7,), -1, dtype=torch.int32, device="cuda")
        L.check(L.lib.wam_peak_normalize(7, n, L.ptr(src), L.ptr(out), L.ptr(silent), zero_silent,
                                         L.stream_of(src.device)))
        ref, ref_silent = R.peak_normalize_ref(x, zero_silent)
        got = out.cpu().numpy()
        assert silent.cpu().tolist() == ref_silent.tolist() == [0, 0, 0, 1, 1, 0, 0]
        R.assert_bits(got, ref, "peak_normalize n=%d zero_silent=%d in_place=%d" % (n, zero_silent, in_place))
        if zero_silent:
            assert np.array_equal(got[3], x[3]) and np.array_equal(got[4], x[4])
        else:
            assert np.isnan(got[3]).all() and np.isnan(got[4, n // 2])
        assert got[0, 0] == 1.0 and got[1, -1] == 1.0 and (got[2] > 0).all()
        if not in_place:
            assert torch.equal(src, dev(x))


# ------------------------------------------------------------------------------ the class
def make_eval(name, inject=True, **kw):
    from wam_amd.evaluation import Eval1DWAM
    case = CASES[name]
    c = ctor_kw(case)
    ev = Eval1DWAM(make_model().cuda(), 128, c["wavelet"], c["J"], c["method"], c["mode"], None, False, c["n_mels"],
                   c["n_fft"], c["sample_rate"], c["n_samples"], **kw)
    if inject:
        ev.grad_wams = golden_grad_wams(name)
    return ev


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern %s vs %s" % (what, got, want)
    if np.isfinite(want).any():
        d = float(np.nanmax(np.abs(got - want)))
        print("[eval1d] %s: max |d| = %.3e" % (what, d))
        return d
    return 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_class_against_the_reference_goldens(L, name):
    """Eval1DWAM(tie_order='numpy') with the golden grad_wams injected vs the reference's numbers:
    NaN pattern equal; curves, scores and faithfulness of spectra within R.BAR; input fidelity's
    arg-max lists equal. From the goldens: the top two logits behind every arg-max are at least 0.03 apart (300 bars)."""
    d = npz(G)
    x, y = make_inputs(CASES[name])
    ev = make_eval(name, tie_order="numpy")
    for target in TARGETS:
        for mode in MODES:
            for n_iter in N_ITERS:
                scores = getattr(ev, mode)(x, y, target, n_iter)
                curves = ev.insertion_curves if mode == "insertion" else ev.deletion_curves
                key = "%s_%s_%s_n%d" % (name, target, mode, n_iter)
                want = d[key + "_curves"]
                dp = close(curves, want, key + "_curves")
                WORST["dp"] = max(WORST["dp"], dp)
                assert dp <= R.BAR, (key, dp)
                ds = close(scores, d[key + "_scores"], key + "_scores")
                WORST["dscore"] = max(WORST["dscore"], ds)
                assert ds <= R.BAR, (key, ds)
        ff = ev.faithfulness_of_spectra(x, y, target)
        dff = close(ff, d["%s_ff_%s" % (name, target)], "%s_ff_%s" % (name, target))
        WORST["dff"] = max(WORST["dff"], dff)
        assert dff <= R.BAR, (name, target, dff)
        logits = np.sort(d["%s_fidlogits_%s" % (name, target)][:, 1:, :], axis=2)
        assert (logits[..., -1] - logits[..., -2]).min() >= 0.03
        assert ev.input_fidelity(x, y, target) == d["%s_fid_%s" % (name, target)].tolist()
    assert isinstance(scores, list) and len(ev.deletion_curves) == N_CLIPS
    assert np.array_equal(ev.grad_wams[0], d[name + "_gw_mel"])   # the injected grad_wams were used, not recomputed


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_stable_tie_order_equals_numpy(L, name, mode):
    """No tie of the goldens straddles a threshold, so the device's stable ranking selects the same
    masks as np.argsort: the curves are equal (every case, both targets, n_iter 4 and 7)."""
    x, y = make_inputs(CASES[name])
    a, b = make_eval(name, tie_order="stable"), make_eval(name, tie_order="numpy")
    for target in TARGETS:
        for n_iter in N_ITERS:
            getattr(a, mode)(x, y, target, n_iter), getattr(b, mode)(x, y, target, n_iter)
            ca, cb = getattr(a, mode + "_curves"), getattr(b, mode + "_curves")
            assert np.array_equal(np.array(ca), np.array(cb), equal_nan=True), (target, n_iter)


@pytest.mark.parametrize("name", ["k4096", "pad4002"])
def test_silent_zero_gives_finite_scores(L, name):
    """silent='zero': the silent row stays silence, every wavelet-target score is finite and equals
    the restatement run with the same rule, within the bar."""
    case = CASES[name]
    x, y = make_inputs(case)
    ev = make_eval(name, tie_order="numpy", silent="zero")
    rules = R.Rules(silent="zero")
    model = make_model()
    for mode in MODES:
        scores = getattr(ev, mode)(x, y, "wavelet", 4)
        curves = ev.insertion_curves if mode == "insertion" else ev.deletion_curves
        _, want, _ = R.evaluate_auc(model, x.numpy(), y, golden_grad_wams(name), mode, "wavelet", 4, cfg_of(case), rules)
        assert np.isfinite(scores).all() and np.isfinite(np.array(want)).all()
        assert close(curves, want, "%s silent=zero %s" % (name, mode)) <= R.BAR


def test_non_haar_wavelet_raises_the_reference_error(L):
    """db2 at 4,096 samples: bands 514, 514, 1025, 2049 against slices 513 wide -- the reference's
    broadcast ValueError, raised on the host before any launch."""
    from wam_amd.plan import get_plan
    case = dict(CASES["k4096"], wavelet="db2")
    x, y = make_inputs(case)
    from wam_amd.evaluation import Eval1DWAM
    ev = Eval1DWAM(make_model().cuda(), wavelet="db2", J=3, n_mels=32, n_fft=256, sample_rate=16000, n_samples=2)
    p = get_plan(1, (4096,), 3, "db2", "reflect", "cuda")
    ev.grad_wams = (np.zeros((N_CLIPS, 33, 32), np.float32), [np.zeros((N_CLIPS,) + s, np.float32) for s in p.band_shapes])
    with pytest.raises(ValueError, match=r"shapes \(514,\) \(5,513\)"):
        ev.insertion(x, y, "wavelet", 4)


def test_unknown_target_is_a_value_error(L):
    ev = make_eval("k4096")
    x, y = make_inputs(CASES["k4096"])
    with pytest.raises(ValueError, match="'wavelet' or 'melspec'"):
        ev.insertion(x, y, "spectrogram", 4)


def test_eval_batch_does_not_change_the_curves(L):
    """eval_batch = n_iter + 1 (one clip per forward) and 520 (both clips in one): the same curves."""
    name = "shift4004"
    x, y = make_inputs(CASES[name])
    one, both = make_eval(name, tie_order="numpy", eval_batch=8), make_eval(name, tie_order="numpy", eval_batch=520)
    for target in TARGETS:
        one.insertion(x, y, target, 7), both.insertion(x, y, target, 7)
        assert close(one.insertion_curves, both.insertion_curves, "eval_batch %s" % target) <= R.BAR


def test_end_to_end_computes_and_caches_grad_wams(L):
    """No injection: the first call computes grad_wams with the inner WaveletAttribution1D, the
    curves equal the restatement fed those grad_wams (within the bar), and a second call does not
    compute them again. A list of clips is peak-normalised first, as the 1D classes do."""
    name = "torch1030"
    case = CASES[name]
    x, y = make_inputs(case)
    ev = make_eval(name, inject=False, tie_order="numpy")
    calls = []
    inner = ev.gradwam
    ev.gradwam = lambda *a: calls.append(1) or inner(*a)
    scores = ev.deletion(x, y, "melspec", 4)
    assert len(calls) == 1 and ev.grad_wams is not None
    gw = ev.grad_wams
    ev.insertion(x, y, "wavelet", 4)
    assert len(calls) == 1 and ev.grad_wams is gw
    model = make_model()
    for mode, target, curves in (("deletion", "melspec", ev.deletion_curves), ("insertion", "wavelet", ev.insertion_curves)):
        # tie_order='numpy' and the restatement run the same np.argsort on the same values: ties cannot differ
        _, want, _ = R.evaluate_auc(model, x.numpy(), y, gw, mode, target, 4, cfg_of(case))
        assert close(curves, want, "end to end %s %s" % (mode, target)) <= R.BAR
    assert np.isfinite(scores).all()
    as_list = [w.numpy() * 3.0 for w in x]
    ev2 = make_eval(name, tie_order="numpy")
    ev2.deletion(as_list, y, "melspec", 4)
    xn = np.array([w / w.max() for w in as_list]).astype(np.float32)
    ev3 = make_eval(name, tie_order="numpy")
    ev3.deletion(torch.tensor(xn), y, "melspec", 4)
    assert np.array_equal(np.array(ev2.deletion_curves), np.array(ev3.deletion_curves))

