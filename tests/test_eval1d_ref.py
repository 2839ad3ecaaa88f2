"""The numpy restatement of Eval1DWAM (tests/eval1d_ref.py) against the goldens made by the reference's
own class (tests/golden/eval1d_goldens.npz). CPU only.

The restatement and the generator's stand-ins run the same oracle arithmetic (oracle.ptwt_torch,
oracle.dwt.waverec, oracle.melspec, the same torch build's CPU model), so masked coefficients, model
inputs, curves and scores are compared for equality, NaN positions included. The comparators are the
ones the GPU test uses with a bar; here the bar is zero, and five mutants of single reference rules
must be rejected by them.
"""
import numpy as np
import pytest

from tests import eval1d_ref as R
from tests.golden.eval1d_cases import (CASES, GOLDENS as G, INPUT_ROWS, MODES, N_CLIPS, N_ITERS, TARGETS, cfg_of,
                                       golden_grad_wams, golden_masked, make_inputs, make_model, straddling_ties)
from tests.helpers import npz


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def compare(name, rules=R.REFERENCE, targets=TARGETS, n_iters=N_ITERS, extras=True):
    """Every stored number of a case against the restatement under `rules`: the names that differ."""
    d = npz(G)
    case = CASES[name]
    x, y = make_inputs(case)
    model, cfg, gw = make_model(), cfg_of(case), golden_grad_wams(name)
    bad = []
    for target in targets:
        for mode in MODES:
            for n_iter in n_iters:
                keep = {}
                scores, curves, _ = R.evaluate_auc(model, x.numpy(), y, gw, mode, target, n_iter, cfg, rules, keep=keep)
                key = "%s_%s_%s_n%d" % (name, target, mode, n_iter)
                if not same(curves, d[key + "_curves"]):
                    bad.append(key + "_curves")
                if not same(scores, d[key + "_scores"]):
                    bad.append(key + "_scores")
                if target == "wavelet" and n_iter == 4:
                    if not same(np.stack(keep["masked"]), golden_masked(name, mode)):
                        bad.append("%s_masked_%s" % (name, mode))
                    if not same(keep["inputs"][0][list(INPUT_ROWS[mode]), 0], d["%s_inputs_%s" % (name, mode)]):
                        bad.append("%s_inputs_%s" % (name, mode))
        if extras:
            if not same(R.faithfulness_of_spectra(model, x.numpy(), y, gw, target, cfg, rules), d["%s_ff_%s" % (name, target)]):
                bad.append("%s_ff_%s" % (name, target))
            if not same(R.input_fidelity(model, x.numpy(), y, gw, target, cfg, rules), d["%s_fid_%s" % (name, target)]):
                bad.append("%s_fid_%s" % (name, target))
    return bad


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_the_goldens(name):
    assert compare(name) == []


@pytest.mark.parametrize("name", list(CASES))
def test_nan_rows_are_the_silent_rows(name):
    """What the reference was seen to do: the all-zero mask (insertion row 0, deletion row n_iter)
    reconstructs silence and 0 / 0 makes its probability NaN, so every wavelet-target score is NaN --
    except where the pad column keeps one coefficient under insertion (4002 samples). The mel target,
    faithfulness of spectra and input fidelity are finite."""
    d = npz(G)
    for n_iter in N_ITERS:
        ins = d["%s_wavelet_insertion_n%d_curves" % (name, n_iter)]
        dele = d["%s_wavelet_deletion_n%d_curves" % (name, n_iter)]
        want_ins = np.zeros(ins.shape, dtype=bool)
        want_ins[:, 0] = name != "pad4002"
        want_del = np.zeros(dele.shape, dtype=bool)
        want_del[:, n_iter] = True
        assert np.array_equal(np.isnan(ins), want_ins) and np.array_equal(np.isnan(dele), want_del)
        assert np.isnan(d["%s_wavelet_deletion_n%d_scores" % (name, n_iter)]).all()
        assert np.isnan(d["%s_wavelet_insertion_n%d_scores" % (name, n_iter)]).all() == (name != "pad4002")
        for mode in MODES:
            assert np.isfinite(d["%s_melspec_%s_n%d_curves" % (name, mode, n_iter)]).all()
    for target in TARGETS:
        assert np.isfinite(d["%s_ff_%s" % (name, target)]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_no_tie_straddles_a_threshold(name):
    """The goldens' rankings have ties, none across a threshold (n_iter 2, 4, 7): the masks do not
    depend on the tie order of the sort."""
    mel, grads = golden_grad_wams(name)
    for s in range(N_CLIPS):
        for values in (np.abs(np.concatenate([g[s] for g in grads])), mel[s]):
            for n_iter in (2,) + tuple(N_ITERS):
                assert straddling_ties(values, n_iter) == []


def test_float32_synthesis_spread_is_the_recorded_d32():
    """d32: the worst |delta p| over the golden cases between the float64 restatement and the one
    whose synthesis and normalisation run in float32 (wavelet target, both modes, n_iter 2, 4, 7).
    Measured 5.96e-8; R.BAR = max(1e-4, 4 * d32) stays 1e-4 as long as d32 <= 2.5e-5."""
    worst = 0.0
    for name, case in CASES.items():
        x, y = make_inputs(case)
        model, cfg, gw = make_model(), cfg_of(case), golden_grad_wams(name)
        for mode in MODES:
            for n_iter in (2,) + tuple(N_ITERS):
                _, c64, _ = R.evaluate_auc(model, x.numpy(), y, gw, mode, "wavelet", n_iter, cfg)
                _, c32, _ = R.evaluate_auc(model, x.numpy(), y, gw, mode, "wavelet", n_iter, cfg, syn_dtype=np.float32)
                c64, c32 = np.array(c64, dtype=np.float64), np.array(c32, dtype=np.float64)
                assert np.array_equal(np.isnan(c64), np.isnan(c32))
                worst = max(worst, float(np.nanmax(np.abs(c64 - c32))))
    print("[eval1d] d32 = %.3e" % worst)
    assert worst <= 4 * R.D32 and R.BAR == 1e-4


MUTANTS = {
    # offsets from the bands' running lengths instead of r: differs where int(L / 2^j) is not a band edge
    "running_offsets": ("shift4004", R.Rules(offsets="running"), ("wavelet",), "shift4004_masked_insertion"),
    # the pad column only exists at 4002 samples
    "pad_swapped": ("pad4002", R.Rules(pad_swapped=True), ("wavelet",), "pad4002_masked_insertion"),
    "wavelet_without_abs": ("k4096", R.Rules(wavelet_abs=False), ("wavelet",), "k4096_masked_deletion"),
    "mel_with_abs": ("k4096", R.Rules(mel_abs=True), ("melspec",), "k4096_melspec_insertion_n4_curves"),
    # n_comp * n_iter < len at n_iter = 7 (the mel ranking has 33 * 32 = 1056 slots, 7 * 150 = 1050): the
    # unforced last mask misses six slots
    "last_mask_not_full": ("k4096", R.Rules(force_last=False), ("melspec",), "k4096_melspec_insertion_n7_curves"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_comparators_reject_mutants(mutant):
    name, rules, targets, must_differ = MUTANTS[mutant]
    bad = compare(name, rules, targets=targets, extras=False)
    assert must_differ in bad, (mutant, bad)


def test_running_offsets_mutant_is_invisible_at_a_dyadic_length():
    """At 4096 samples the bands' running lengths are r itself: why the mutants above pick their cases."""
    assert compare("k4096", R.Rules(offsets="running"), targets=("wavelet",), n_iters=(4,), extras=False) == []


def test_db2_raises_the_reference_broadcast_error():
    case = dict(CASES["k4096"], wavelet="db2")
    x, _ = make_inputs(case)
    lens = [514, 514, 1025, 2049]
    grads = [np.zeros((N_CLIPS, n), dtype=np.float32) for n in lens]
    with pytest.raises(ValueError, match=r"shapes \(514,\) \(5,513\)"):
        R.wavelet_inputs(x[0].numpy(), grads, 0, "insertion", 4, cfg_of(case))
    from wam_amd.evaluation import coeff_slot_map
    with pytest.raises(ValueError, match=r"shapes \(514,\) \(5,513\)"):    # the product's host check: the same words
        coeff_slot_map(case["L"], case["J"], lens, 5)


@pytest.mark.parametrize("length,J,lens", [(4096, 3, [512, 512, 1024, 2048]), (4002, 3, [501, 501, 1001, 2001]),
                                           (4004, 3, [501, 501, 1001, 2002]), (1030, 2, [258, 258, 515]),
                                           (4000, 3, [500, 500, 1000, 2000]), (4006, 3, [501, 501, 1002, 2003]),
                                           (4098, 3, [513, 513, 1025, 2049]), (37, 2, [10, 10, 19])])
def test_host_slot_map_is_the_reference_slicing(length, J, lens):
    """Eval1DWAM's host slot map (the `pos` of wam_rank_mask_coeffs) against the restatement's band
    slicing, at the lengths the reference was seen to run: slot k of the map picks column k of the
    mask, -1 the pad column. db2 at 4,096 samples raises the reference's error."""
    from wam_amd.evaluation import coeff_slot_map
    pos = coeff_slot_map(length, J, lens)
    K = sum(lens)
    masks = np.arange(1, K + 1, dtype=np.float64)[None, :]           # column c holds c + 1
    want = np.concatenate([m[0] for m in R.band_masks(masks, length, J, lens, deletion=True)])   # pad column: 0
    assert np.array_equal(np.where(pos < 0, 0, pos + 1), want)
    with pytest.raises(ValueError, match=r"shapes \(514,\) \(5,513\)"):
        coeff_slot_map(4096, 3, [514, 514, 1025, 2049], 5)


# ------------------------------------------------------------------------------ C-ABI references
def test_cabi_references_agree_with_the_restatement():
    """rank_mask_coeffs_ref fed the slot map of the reference's slices gives the restatement's
    masked coefficients (pad4002, both modes); rank_mask_rows_ref gives its mel-target inputs;
    peak_normalize_ref its float32 normalisation."""
    name = "pad4002"
    case, d = CASES[name], npz(G)
    mel, grads = golden_grad_wams(name)
    lens = [g.shape[1] for g in grads]
    off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    K = off[-1]
    slices = R.band_slices(case["L"], case["J"], lens)
    pos = np.concatenate([np.concatenate([np.arange(a, min(b, K)), -np.ones(n - (min(b, K) - a), dtype=np.int64)])
                          for (a, b), n in zip(slices, lens)])
    assert (pos == -1).sum() == 1 and pos[off[1] + lens[1] - 1] == -1
    g = np.abs(np.stack([np.concatenate([b[s] for b in grads]) for s in range(N_CLIPS)]))
    order = np.stack([np.argsort(v)[::-1] for v in g])
    rank = np.empty_like(order)
    for s in range(N_CLIPS):
        rank[s, order[s]] = np.arange(K)
    item = d[name + "_coeffs"]                                                # [clips, K] band after band
    flat = np.concatenate([item[:, off[b]:off[b + 1]].reshape(-1) for b in range(len(lens))])
    for mode in MODES:
        out = R.rank_mask_coeffs_ref(off, N_CLIPS, flat, rank, pos, 4, int(K / 4), mode == "deletion")
        got = np.concatenate([out[N_CLIPS * 5 * off[b]:N_CLIPS * 5 * off[b + 1]].reshape(N_CLIPS, 5, lens[b])
                              for b in range(len(lens))], axis=2)
        R.assert_bits(got, golden_masked(name, mode), "rank_mask_coeffs_ref %s" % mode)
    x, _ = make_inputs(case)
    cfg = cfg_of(case)
    source = R.compute_melspec(x.numpy(), cfg["n_fft"], cfg["sample_rate"], cfg["n_mels"]).squeeze(1).numpy()
    n = source[0].size
    mo = np.stack([np.argsort(m, axis=None)[::-1] for m in mel])
    mrank = np.empty_like(mo)
    for s in range(N_CLIPS):
        mrank[s, mo[s]] = np.arange(n)
    for mode in MODES:
        rows = R.rank_mask_rows_ref(source.reshape(N_CLIPS, n), mrank, 7, int(n / 7), mode == "deletion")
        for s in range(N_CLIPS):
            want = R.melspec_inputs(mel[s], source[s], mode, 7).numpy().reshape(8, n)
            R.assert_bits(rows[s], want, "rank_mask_rows_ref %s clip %d" % (mode, s))
    rec = np.array([[0.5, -2.0, 1.5, 0.25], [0.0, 0.0, 0.0, 0.0], [-3.0, -1.0, -2.0, -1.5], [-1.0, 0.0, -2.0, 0.0]],
                   dtype=np.float32)
    out, silent = R.peak_normalize_ref(rec, 0)
    assert silent.tolist() == [0, 1, 0, 1]
    assert np.array_equal(out[0], rec[0] / np.float32(1.5)) and np.isnan(out[1]).all()
    assert np.array_equal(out[2], rec[2] / np.float32(-1.0)) and np.isneginf(out[3][[0, 2]]).all()
    out, silent = R.peak_normalize_ref(rec, 1)
    assert np.array_equal(out[1], rec[1]) and np.array_equal(out[3], rec[3]) and silent.tolist() == [0, 1, 0, 1]
