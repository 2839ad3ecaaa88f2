"""The numpy restatement of WAMAnalyzer2D (tests/analyzer_ref.py) against the goldens the reference's own
helpers produced (tests/golden/analyzer_goldens.npz, real PyWavelets 1.1.1), on the CPU; and the
mutants: every single rule of the restatement switched off must be rejected by the same comparators
the device tests use.

Comparators: thresholds and masks exact; float images by R.float_distance <= R.D32; uint8 images by
circular grey-level distance <= 1 with the share of pixels at non-zero distance <= R.CAP (a wrap
boundary turns one ulp into 255 levels, hence circular). The restatement alone has to stay under a
quarter of the cap, checked at 64^2 and 224^2 (at 32^2 the cap is three pixels).
Measured (float64 oracle.dwt against float32 pywt): worst float distance 4.77e-7 (the 64^2 partial image at
q = 0), which is what R.D32 records; uint8 images: 1 of 12,288 values at 64^2 (8.1e-5) and 3 of 50,176 at
224^2 (6.0e-5) one grey level apart, none further.
"""
import numpy as np
import pytest

from tests import analyzer_ref as R
from tests.golden.analyzer_cases import EPS, GOLDENS, LEVELS, PARTIAL, QUIRK, key, make_image, make_map
from tests.helpers import npz

SWEEP = np.concatenate([[0.0, 1.0], np.random.RandomState(11).uniform(size=2000)])   # quantiles with awkward fractions
ALL_Q = dict(list(PARTIAL.items()) + list(QUIRK.items()))


def bits(packed, shape):
    return np.unpackbits(packed)[:int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.fixture(scope="module")
def partials():
    """The restatement's (image, mask, threshold) for every stored case and quantile, computed once."""
    out = {}
    for name, (size, J, seed, chans, qs) in ALL_Q.items():
        img, wam = make_image(size, seed), make_map(size, seed)
        for q in qs:
            out[name, q] = R.partial_image(img, wam, q, J)
    return out


@pytest.fixture(scope="module")
def levels():
    return {name: R.disentangled(make_map(size, seed), make_image(size, seed), J, EPS)
            for name, (size, J, seed, chans) in LEVELS.items()}


def test_thresholds_and_masks_are_exact(partials):
    g = npz(GOLDENS)
    for name, (size, J, seed, chans, qs) in ALL_Q.items():
        wam = make_map(size, seed)
        for k, q in enumerate(qs):
            _, mask, t = partials[name, q]
            assert t == g[key("thr", name)][k], (name, q)
            want = bits(g[key("pmask", name, q)], (size, size))
            assert np.array_equal(mask, want * wam), (name, q)
    # q = 0 and q = 1: the threshold is an element of the map (g = 0), kept by >=
    assert partials["s32", 0.0][2] == make_map(32, 3201).min() and (partials["s32", 0.0][1] != 0).all()
    assert partials["s32", 1.0][2] == make_map(32, 3201).max() and (partials["s32", 1.0][1] != 0).sum() == 1


def test_quantile_equals_numpy():
    """The restated quantile equals np.quantile bit for bit on a sweep that takes both _lerp branches."""
    wam = make_map(32, 3201)
    for q in SWEEP:
        assert R.quantile(wam, q) == np.quantile(wam, q), q


def test_float_images_within_d32(partials, levels):
    g = npz(GOLDENS)
    worst = 0.0
    for name, (size, J, seed, chans, qs) in PARTIAL.items():
        for q in qs:
            d = R.float_distance(partials[name, q][0][:, :, list(chans)], g[key("partial", name, q)])
            print("[analyzer ref] partial %s q=%.2f: d = %.3e" % (name, q, d))
            worst = max(worst, d)
    for name, (size, J, seed, chans) in LEVELS.items():
        d = R.float_distance(levels[name][0][..., list(chans)], g[key("levels", name)])
        print("[analyzer ref] levels %s: d = %.3e" % (name, d))
        worst = max(worst, d)
    print("[analyzer ref] worst float distance %.3e (D32 = %.1e)" % (worst, R.D32))
    assert worst <= R.D32


def test_level_masks_are_exact(levels):
    g = npz(GOLDENS)
    for name, (size, J, seed, chans) in LEVELS.items():
        want = bits(g[key("lmask", name)], (J + 1, size, size)) * make_map(size, seed)[None]
        assert np.array_equal(levels[name][1], want), name
        assert levels[name][0].shape == (J + 1, size, size, 3) and levels[name][0].dtype == np.float64


def test_uint8_images_within_a_quarter_of_the_cap(partials):
    g = npz(GOLDENS)
    for name, (size, J, seed, chans, qs) in QUIRK.items():
        for q in qs:
            u8 = R.quantize(partials[name, q][0])
            mx, share = R.u8_compare(u8[:, :, list(chans)], g[key("quirk", name, q)])
            print("[analyzer ref] quirk %s q=%.2f: max circular distance %d, share %.2e" % (name, q, mx, share))
            assert mx <= 1 and share <= R.CAP / 4, (name, q, mx, share)
            # the quirk is live: a sizeable share of the grey levels wrapped
            assert (R.quantize(partials[name, q][0], R.Rules(cast="saturate")) != u8).mean() > 0.1


def test_wrapping_cast_examples():
    assert R.wrap_u8(np.float32([-3.7, 300.7, 1000.3, np.nan, np.inf, -np.inf, 3e9, 255.9, -0.5])).tolist() == \
        [253, 44, 232, 0, 0, 0, 0, 255, 0]


# ------------------------------------------------------------------------------ mutants
def u8_ok(got, want):
    mx, share = R.u8_compare(got, want)
    return mx <= 1 and share <= R.CAP


def test_mutant_strict_comparison_is_rejected(partials):
    img, wam = make_image(32, 3201), make_map(32, 3201)
    _, mask, _ = R.partial_image(img, wam, 0.0, 2, rules=R.Rules(ge=False))
    assert not np.array_equal(mask, partials["s32", 0.0][1])
    g = npz(GOLDENS)
    assert not np.array_equal(mask, bits(g[key("pmask", "s32", 0.0)], (32, 32)) * wam)


def test_mutant_mosaic_layout_is_rejected():
    g = npz(GOLDENS)
    size, J, seed, chans, qs = PARTIAL["s64"]
    image, _, _ = R.partial_image(make_image(size, seed), make_map(size, seed), 0.7, J, rules=R.Rules(layout="mosaic"))
    assert R.float_distance(image[:, :, list(chans)], g[key("partial", "s64", 0.7)]) > 1e3 * R.D32


def test_mutant_shifted_level_region_is_rejected():
    g = npz(GOLDENS)
    size, J, seed, chans = LEVELS["s32"]
    _, filtered = R.disentangled(make_map(size, seed), make_image(size, seed), J, EPS, rules=R.Rules(level_shift=1))
    assert not np.array_equal(filtered != 0, bits(g[key("lmask", "s32")], (J + 1, size, size)))


def test_mutant_region_minimum_is_rejected():
    """The maps are strictly positive, so the minimum over the region alone is above the array's 0."""
    g = npz(GOLDENS)
    size, J, seed, chans = LEVELS["s32"]
    images, _ = R.disentangled(make_map(size, seed), make_image(size, seed), J, EPS, rules=R.Rules(level_min="region"))
    assert R.float_distance(images[..., list(chans)], g[key("levels", "s32")]) > 1e3 * R.D32


@pytest.mark.parametrize("rules", [R.Rules(quant="minmax"), R.Rules(cast="saturate")], ids=["minmax", "saturate"])
def test_mutant_quantisation_is_rejected(partials, rules):
    g = npz(GOLDENS)
    size, J, seed, chans, qs = QUIRK["s64u"]
    for q in qs:
        assert not u8_ok(R.quantize(partials["s64u", q][0], rules)[:, :, list(chans)], g[key("quirk", "s64u", q)])


def test_mutant_single_branch_lerp_is_rejected():
    wam = make_map(32, 3201)
    mutant = R.Rules(lerp_second=False)
    differ = [q for q in SWEEP if R.quantile(wam, q, mutant) != np.quantile(wam, q)]
    assert differ and all((1023 * q) % 1 >= 0.5 for q in differ)


def test_db2_is_the_reference_broadcast_error():
    with pytest.raises(ValueError, match=r"shapes \(37,37\) \(32,32\)"):
        R.partial_image(make_image(32, 1), make_map(32, 1), 0.5, 2, wavelet="db2")


# ------------------------------------------------------------------------------ C-ABI references
def test_quantize_ref_matches_the_restatement():
    """quantize_ref (planar, per image) and quantize (one HWC image) are the same rule."""
    rs = np.random.RandomState(5)
    hwc = rs.standard_normal((16, 16, 3)).astype(np.float32) * 3
    u8, out = R.quantize_ref(np.moveaxis(hwc, 2, 0).reshape(1, 3, -1), 1, R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert np.array_equal(np.moveaxis(u8[0].reshape(3, 16, 16), 0, 2), R.quantize(hwc))
    u0, _ = R.quantize_ref(np.moveaxis(hwc, 2, 0).reshape(1, 3, -1), 0)
    assert np.array_equal(np.moveaxis(u0[0].reshape(3, 16, 16), 0, 2), R.quantize(hwc, R.Rules(quant="minmax", cast="saturate")))
    assert out.dtype == np.float32 and out.shape == (1, 3, 256)


def test_threshold_mask_ref_matches_the_restatement():
    """threshold_mask_coeffs_ref on pywt's positions reproduces arr * (map >= t) and the level masks."""
    size, J = 16, 2
    rs = np.random.RandomState(9)
    img, wam = rs.uniform(size=(size, size)), make_map(size, 9)
    coeffs = R.dwt.wavedec2(img, "haar", J, mode="symmetric")
    arr, sl = R.to_array(coeffs)
    flat = [coeffs[0]] + [b for lv in coeffs[1:] for b in lv]
    off = np.concatenate([[0], np.cumsum([b.size for b in flat])]).tolist()
    idx = np.arange(size * size).reshape(size, size)
    pos = np.concatenate([b.reshape(-1) for b in ([idx[sl[0]]] + [idx[s] for lv in sl[1:] for s in lv])]).astype(np.int32)
    cf = np.concatenate([b.reshape(-1) for b in flat]).astype(np.float32)
    thr = np.array([R.quantile(wam, q) for q in (0.0, 0.5, 1.0)])
    out = R.threshold_mask_coeffs_ref(off, 1, 1, cf, pos, size, wam.reshape(1, -1), 3, thr, 3)
    for q in range(3):
        want = (arr * (wam >= thr[q])).astype(np.float32)
        got = np.concatenate([out[3 * off[b] + q * (off[b + 1] - off[b]):3 * off[b] + (q + 1) * (off[b + 1] - off[b])]
                              for b in range(len(off) - 1)])
        assert np.array_equal(got, want.reshape(-1)[pos])
    filt = R.levelized_masks(wam, J)
    lthr = np.array([filt[l].min() + EPS for l in range(J + 1)])
    out = R.threshold_mask_coeffs_ref(off, 1, 1, cf, pos, size, wam.reshape(1, -1), J + 1, lthr, J + 1, 1,
                                      R.level_edges(size, J), 1)
    for l in range(J + 1):
        want = (arr * (filt[l] > lthr[l])).astype(np.float32)
        got = np.concatenate([out[(J + 1) * off[b] + l * (off[b + 1] - off[b]):(J + 1) * off[b] + (l + 1) * (off[b + 1] - off[b])]
                              for b in range(len(off) - 1)])
        assert np.array_equal(got, want.reshape(-1)[pos])
