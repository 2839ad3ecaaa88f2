"""wam_amd.utils on the GPU: wam_level_stats and wam_mask_iou (wam_amd/csrc/scalestats.hip) against what the
reference's own utils.py (real scipy.ndimage.zoom) and notebook cell produced
(tests/golden/scalestats_goldens.npz, inputs regenerated from tests/golden/scalestats_cases.py).

Bars (tests/scalestats_ref.py, u = 2^-53): abs_sums relative (2 n + 8) u with n the block's element count;
var_map absolute (128 + 16 J) u max(map^2); mean_var that plus 2 T^2 u mean_var. Integer counts, IoU floats,
rankings and everything computed twice are compared exactly. Every comparison prints its worst deviation
in units of its bar before it asserts.
"""
import numpy as np
import pytest
import torch

import testmodels
from tests import scalestats_ref as R
from tests.golden import scalestats_cases as C
from tests.helpers import npz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def U():
    from wam_amd import utils
    return utils


@pytest.fixture(scope="module")
def maps():
    return {name: C.make_maps(H, N, seed) for name, (H, J, N, seed, stored) in C.LEVEL_CASES.items()}


def block_counts(H, J):
    return np.array([n * n for n in R.detail_sides(H, J)] + [(H // 2 ** J) ** 2], dtype=np.float64)


# ---------------------------------------------------------------------------------- level statistics

@pytest.mark.parametrize("name", list(C.LEVEL_CASES))
def test_level_shares_vs_reference(U, maps, name):
    H, J, N, seed, stored = C.LEVEL_CASES[name]
    g = npz(C.GOLDENS)
    abs_dev, _, _ = U._level_stats(U._maps_dev(maps[name]), J, want_abs=True)
    got = abs_dev.cpu().numpy()
    want = g[C.level_key("abs", name)]
    assert got.shape == want.shape == (N, J + 1)
    bar = np.array([R.abs_sum_rtol(n) for n in block_counts(H, J)])[None, :] * np.abs(want)
    dev = np.abs(got - want)
    print("abs_sums %s: worst deviation %.3g u relative, %.3g of the bar"
          % (name, (dev / np.maximum(np.abs(want), 1e-300)).max() / R.U, (dev / np.maximum(bar, 1e-300)).max()))
    assert (dev <= bar).all()
    shares = U.level_shares(maps[name], J)
    assert shares.shape == (N, J + 1) and shares.dtype == np.float64
    # the division is numpy's on the host copy: each share inherits the sums' relative bar twice (numerator and
    # total, both sums of at most H^2 terms)
    want_shares = g[C.level_key("shares", name)]
    assert (np.abs(shares - want_shares) <= 2 * R.abs_sum_rtol(H * H) * want_shares).all()
    assert np.array_equal(shares, np.array(U._shares(got)))


@pytest.mark.parametrize("size", C.SIZES)
@pytest.mark.parametrize("name", list(C.LEVEL_CASES))
def test_pixelwise_variance_vs_reference(U, maps, name, size):
    H, J, N, seed, stored = C.LEVEL_CASES[name]
    g = npz(C.GOLDENS)
    T = R.target_side(H, J, size)
    for i, m in enumerate(maps[name]):
        mean_var, var_map = U.get_mean_pixelwise_variance(m, J, size=size)
        assert isinstance(mean_var, float) and var_map.shape == (T, T) and var_map.dtype == np.float64
        want_mean = float(g[C.level_key("mvar", name, size)][i])
        bar = R.mean_var_atol(J, m, T, want_mean)
        print("mean_var %s %s [%d]: deviation %.3g u max(map^2), %.3g of the bar"
              % (name, size, i, abs(mean_var - want_mean) / (R.U * np.max(m ** 2)), abs(mean_var - want_mean) / bar))
        assert abs(mean_var - want_mean) <= bar
        if size in stored:
            want = g[C.level_key("vmap", name, size)][i]
            dev = float(np.abs(var_map - want).max())
            print("var_map %s %s [%d]: worst deviation %.3g u max(map^2), %.3g of the bar"
                  % (name, size, i, dev / (R.U * np.max(m ** 2)), dev / R.var_atol(J, m)))
            assert dev <= R.var_atol(J, m)
        if J == 1:
            assert mean_var == 0.0 and not var_map.any()   # a single level: exactly 0.0


@pytest.mark.parametrize("name", C.RANK_CASES)
def test_rank_images_vs_reference(U, maps, name):
    H, J, N, seed, stored = C.LEVEL_CASES[name]
    g = npz(C.GOLDENS)
    for size in C.SIZES:
        ranking = U.rank_images(maps[name], J, size=size)
        assert [set(r) for r in ranking] == [{"image_index", "mean_pixelwise_variance"}] * N
        assert [r["image_index"] for r in ranking] == list(g[C.level_key("rank", name, size)])
        want = g[C.level_key("mvar", name, size)]
        for r in ranking:
            i = r["image_index"]
            assert isinstance(r["mean_pixelwise_variance"], float)
            assert abs(r["mean_pixelwise_variance"] - want[i]) <= R.mean_var_atol(J, maps[name][i],
                                                                                  R.target_side(H, J, size), want[i])
            # one launch for all images == one launch per image, bit for bit
            assert r["mean_pixelwise_variance"] == U.get_mean_pixelwise_variance(maps[name][i], J, size=size)[0]


def test_rank_ties_keep_image_order(U, maps):
    m = maps["s32n5"]
    twins = np.stack([m[1], m[0], m[1], m[0]])
    got = [r["image_index"] for r in U.rank_images(twins, 3)]
    mv = [R.mean_variance(x, 3) for x in twins]
    assert got == ([0, 2, 1, 3] if mv[0] > mv[1] else [1, 3, 0, 2])


def test_errors_are_the_references(U):
    with pytest.raises(AssertionError, match="grad_wam must be square"):
        U.get_mean_pixelwise_variance(torch.zeros(8, 6, dtype=torch.float64, device="cuda"), 2)
    with pytest.raises(AssertionError, match="grad_wam must be square"):
        U.rank_images(np.zeros((2, 8, 6)), 2)
    with pytest.raises(ValueError, match="size must be 'maximal' or 'minimal'"):
        U.rank_images(np.zeros((2, 8, 8)), 2, size="median")
    with pytest.raises(ZeroDivisionError):
        U.get_mean_pixelwise_variance(torch.zeros(4, 4, dtype=torch.float64, device="cuda"), 4)


def test_same_bits_twice_and_from_device_input(U, maps):
    for name in ("s224n3", "s100", "s32n5"):
        H, J = C.LEVEL_CASES[name][:2]
        host = maps[name]
        dev = torch.as_tensor(host).cuda()
        for size in C.SIZES:
            a = U._level_stats(dev, J, size, want_abs=True, want_map=True, want_mean=True)
            b = U._level_stats(dev, J, size, want_abs=True, want_map=True, want_mean=True)
            c = U._level_stats(U._maps_dev(host), J, size, want_abs=True, want_mean=True)   # no map stored
            for x, y in zip(a, b):
                assert torch.equal(x, y)
            assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2]) and c[1] is None
            r_host, r_dev = U.rank_images(host, J, size=size), U.rank_images(dev, J, size=size)
            assert r_host == r_dev
            m_host, m_dev = U.get_mean_pixelwise_variance(host[0], J, size), U.get_mean_pixelwise_variance(dev[0], J, size)
            assert m_host[0] == m_dev[0] and np.array_equal(m_host[1], m_dev[1])
        assert np.array_equal(U.level_shares(host, J), U.level_shares(dev, J))


def test_one_image_of_a_batch_equals_the_image_alone(U, maps):
    """The partial sums of an image do not depend on its neighbours in the launch."""
    m = torch.as_tensor(maps["s224n3"]).cuda()
    whole = U._level_stats(m, 3, "maximal", want_abs=True, want_map=True, want_mean=True)
    for i in range(3):
        one = U._level_stats(m[i:i + 1].contiguous(), 3, "maximal", want_abs=True, want_map=True, want_mean=True)
        for x, y in zip(whole, one):
            assert torch.equal(x[i:i + 1], y)


# ---------------------------------------------------------------------------------- explainer hand-off

@pytest.fixture(scope="module")
def explained():
    from PIL import Image
    from wam_amd.wam_2D import WaveletAttribution2D
    rs = np.random.RandomState(77)
    images = [Image.fromarray(rs.randint(0, 256, size=(224, 224, 3)).astype(np.uint8)) for _ in range(3)]
    model = testmodels.TinySmooth2D().cuda()
    ex = WaveletAttribution2D(model, wavelet="haar", J=3, method="smooth", mode="reflect", n_samples=2)
    transform = lambda im: torch.from_numpy(np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0)  # noqa: E731
    return images, model, ex, transform


def test_map_device_is_the_returned_map(U, explained):
    from wam_amd.wam_2D import WaveletAttribution2D
    images, model, ex, transform = explained
    assert WaveletAttribution2D(model, wavelet="haar", J=3, n_samples=2).map_device is None
    got = U.get_explanations_for_image(images[0], model, ex, transform, "cuda", 3)
    assert got.shape == (224, 224) and got.dtype == np.float64
    dev = ex.map_device
    assert dev.is_cuda and dev.dtype == torch.float64 and tuple(dev.shape) == (1, 224, 224)
    assert np.array_equal(dev[0].cpu().numpy(), got)
    with pytest.raises(AttributeError):
        ex.map_device = None


def test_gradients_attribution_on_levels(U, explained, capsys):
    images, model, ex, transform = explained
    got = U.get_gradients_attribution_on_levels(images, model, ex, transform, "cuda", 3)
    assert capsys.readouterr().out == ""          # the reference's print(k) is dropped
    expl = [U.get_explanations_for_image(im, model, ex, transform, "cuda", 3) for im in images]
    assert isinstance(got, list) and len(got) == 3
    for g_, e in zip(got, expl):
        want = R.shares(e, 3)
        assert g_.shape == (4,) and g_.dtype == np.float64 and abs(g_.sum() - 1.0) <= 8 * R.U
        assert (np.abs(g_ - want) <= 2 * R.abs_sum_rtol(224 * 224) * want).all(), (g_, want)
    both = U.get_multiple_grad_attr(images[:2], [model, model], [ex, ex], transform, "cuda", 3)
    assert len(both) == 2 and all(np.array_equal(a, b) for a, b in zip(both[0], got[:2]))
    mean = U.get_mean_across_images(both)
    assert np.array_equal(mean[0], np.mean(np.array(got[:2]), axis=0))


def test_grad_reprojection_and_wavelet_iou(U, explained):
    images, model, ex, transform = explained
    expl = U.get_explanations_for_image(images[1], model, ex, transform, "cuda", 3)
    got = U.get_grad_reprojection(expl, ex, 3, "haar", "smooth")
    want = ex.reproject_wam(expl.reshape((1, 224, 224)), 3).mean(axis=1).squeeze()
    assert got.shape == (224, 224) and np.array_equal(got, want)
    ps = [0.1, 0.3]
    # the notebook's METHOD: the reference's SmoothGrad frame takes no wavelet but haar at 224
    res = U.get_iou_between_wavelets(images[1], ["haar", "db2", "sym4"], ps, model=model, transform=transform,
                                     device="cuda", J=3, method="integratedgrad")
    one = U.get_iou_between_wavelets(images[1], ["haar", "db2", "sym4"], 0.3, model=model, transform=transform,
                                     device="cuda", J=3, method="integratedgrad")
    assert res.shape == (2,) and res.dtype == np.float64 and np.ndim(one) == 0 and one == res[1]
    assert ((res > 0) & (res <= 1)).all()


def test_grad_reprojection_ignores_the_explainers_approx_flag(U, explained):
    """The notebook calls reproject_wam(explanation, levels) with its own approx_coeffs default, False: `levels`
    planes whatever the explainer was built with; more levels than J leave zero planes in the mean; fewer raise."""
    from wam_amd.wam_2D import WaveletAttribution2D
    images, model, ex, transform = explained
    ex_a = WaveletAttribution2D(model, wavelet="haar", J=3, method="smooth", mode="reflect", n_samples=2,
                                approx_coeffs=True)
    expl = U.get_explanations_for_image(images[2], model, ex_a, transform, "cuda", 3)
    for levels in (3, 4):
        got = U.get_grad_reprojection(expl, ex_a, levels, "haar", "smooth")
        want = ex_a.reproject_wam(expl.reshape(1, 224, 224), levels).mean(axis=1).squeeze()
        assert got.shape == (224, 224) and np.array_equal(got, want), levels
        assert np.array_equal(got, U.get_grad_reprojection(ex_a.map_device, ex, levels, "haar", "smooth"))
    with pytest.raises(IndexError, match="index 2 is out of bounds for axis 1 with size 2"):
        U.get_grad_reprojection(expl, ex_a, 2, "haar", "smooth")
    with pytest.raises(IndexError, match="index 2 is out of bounds for axis 1 with size 2"):
        ex_a.reproject_wam(expl.reshape(1, 224, 224), 2)


def test_empty_device_batch(U):
    assert U.rank_images(torch.zeros(0, 8, 8, dtype=torch.float64, device="cuda"), 2) == []
    out = U._level_stats(torch.zeros(0, 8, 8, dtype=torch.float64, device="cuda"), 2, "maximal", want_abs=True,
                         want_mean=True)
    assert tuple(out[0].shape) == (0, 3) and out[1] is None and tuple(out[2].shape) == (0,)


# ---------------------------------------------------------------------------------- mask agreement

def iou_inputs():
    cases = {k: C.make_iou_maps(*v) for k, v in C.iou_cases().items()}
    cases[C.IOU_TWINS[0]] = C.make_twins(C.IOU_TWINS[1])
    return cases


@pytest.mark.parametrize("name", list(iou_inputs()))
def test_mask_iou_vs_reference(U, name):
    m = iou_inputs()[name]
    g = npz(C.GOLDENS)
    flat = U._flat_maps(m)
    inter, uni = U._mask_counts(flat, U._thresholds(flat, C.PERCENTAGES))
    assert inter.dtype == np.int64 and inter.shape == g["inter_" + name].shape
    assert np.array_equal(inter, g["inter_" + name]) and np.array_equal(uni, g["uni_" + name])
    got = U.mean_pairwise_iou(m, C.PERCENTAGES)
    assert got.dtype == np.float64 and np.array_equal(got, g["miou_" + name])
    assert np.array_equal(U.mean_pairwise_iou(torch.as_tensor(m).cuda(), C.PERCENTAGES), got)
    if name == C.IOU_TWINS[0]:
        assert np.array_equal(got, np.ones(len(C.PERCENTAGES)))


def test_mask_iou_chunks_equal_one_launch(U):
    """The chunked path (M > 16 maps, or more than 16 percentages) against launches within the bounds."""
    name, M, n = C.IOU_CHUNKED
    flat = U._flat_maps(C.make_iou_maps(*C.iou_cases()[name]))
    thr = U._thresholds(flat, C.PERCENTAGES)
    assert U._mask_iou_call(flat, thr)[0] == 3   # WAM_ERR_UNSUPPORTED
    inter, uni = U._mask_counts(flat, thr)
    sub_i, sub_u = U._mask_counts(flat[:16].contiguous(), thr[:16].contiguous())
    cols = [k for k, (i, j) in enumerate((i, j) for i in range(M) for j in range(i + 1, M)) if j < 16]
    assert np.array_equal(inter[:, cols], sub_i) and np.array_equal(uni[:, cols], sub_u)
    many = tuple(np.linspace(0.0, 1.0, 21))      # 21 percentages: two chunks
    few = U.mean_pairwise_iou(flat[:3], many[:16]), U.mean_pairwise_iou(flat[:3], many[16:])
    assert np.array_equal(U.mean_pairwise_iou(flat[:3], many), np.concatenate(few))


def test_mask_iou_large_map_and_nan(U):
    """More than one workgroup and several chunks per workgroup (6 maps x 10 percentages at 224^2, the
    notebook's shape), a length that is no multiple of 64, and NaN pixels, which no threshold selects."""
    rs = np.random.RandomState(5)
    m = np.round(rs.standard_normal((6, 224 * 224 + 37)), 2)     # rounded: ties at the thresholds
    ps = C.PERCENTAGES[:10]
    inter, uni = R.pair_counts(m, ps)
    flat = U._flat_maps(m)
    gi, gu = U._mask_counts(flat, U._thresholds(flat, ps))
    assert np.array_equal(gi, inter) and np.array_equal(gu, uni)
    assert np.array_equal(U.mean_pairwise_iou(m, ps), R.mean_iou(inter, uni))
    thr = U._thresholds(flat, ps)
    holes = flat.clone()
    holes[:, ::7] = float("nan")
    hi, hu = U._mask_counts(holes, thr)
    keep = np.ones(m.shape[1], bool)
    keep[::7] = False
    t = thr.cpu().numpy()
    M = len(m)
    for q in range(len(ps)):
        sel = [(m[i] >= t[i, q]) & keep for i in range(M)]
        pairs = [(i, j) for i in range(M) for j in range(i + 1, M)]
        assert list(hi[q]) == [int((sel[i] & sel[j]).sum()) for i, j in pairs]
        assert list(hu[q]) == [int((sel[i] | sel[j]).sum()) for i, j in pairs]


def test_highest_percentage_mask(U):
    m = C.make_iou_maps(1, 1000, 9)[0].reshape(25, 40)
    for p in (0.0, 0.05, 0.5, 1.0):
        got = U.get_highest_percentage(m, p)
        assert got.dtype == bool and got.shape == m.shape and np.array_equal(got, R.highest_percentage(m, p))
    assert U.get_highest_percentage(m, 0.0).all()
