"""The numpy restatement of the scale statistics and mask agreement (tests/scalestats_ref.py) against
what the reference's own utils.py (real scipy.ndimage.zoom) and notebook cell produced
(tests/golden/scalestats_goldens.npz), on the CPU; the host-only functions of wam_amd.utils; and the
host-side argument checks of the new C entry points.

The restatement follows scipy and numpy operation by operation, so everything here is compared for
EXACT equality. The device tests (tests/test_gpu_scalestats.py) compare the kernels with the same
goldens under the bars of scalestats_ref (abs_sum_rtol, var_atol, mean_var_atol); the mutants below
show what those bars reject: an out-of-bounds coordinate treated as the edge, and another coordinate
formula wherever scipy's own rounds out of bounds (and that they do not see a one-ulp difference of an
in-bounds coordinate).
"""
import ctypes

import numpy as np
import pytest

from tests import scalestats_ref as R
from tests.golden import scalestats_cases as C
from tests.helpers import npz
from wam_amd import _lib, utils


@pytest.fixture(scope="module")
def maps():
    return {name: C.make_maps(H, N, seed) for name, (H, J, N, seed, stored) in C.LEVEL_CASES.items()}


def test_abs_sums_and_shares_are_exact(maps):
    g = npz(C.GOLDENS)
    for name, (H, J, N, seed, stored) in C.LEVEL_CASES.items():
        for i, m in enumerate(maps[name]):
            assert np.array_equal(R.abs_sums(m, J), g[C.level_key("abs", name)][i]), name
            assert np.array_equal(R.shares(m, J), g[C.level_key("shares", name)][i]), name
        assert g[C.level_key("abs", name)].shape == (N, J + 1)


def test_variance_is_exact(maps):
    g = npz(C.GOLDENS)
    for name, (H, J, N, seed, stored) in C.LEVEL_CASES.items():
        for size in C.SIZES:
            T = R.target_side(H, J, size)
            for i, m in enumerate(maps[name]):
                vm = R.variance_map(m, J, size)
                assert vm.shape == (T, T)
                assert float(np.mean(vm)) == g[C.level_key("mvar", name, size)][i], (name, size)
                if size in stored:
                    assert np.array_equal(vm, g[C.level_key("vmap", name, size)][i]), (name, size)


def test_single_level_variance_is_zero(maps):
    g = npz(C.GOLDENS)
    for size in C.SIZES:
        assert not g[C.level_key("vmap", "s64j1", size)].any() and not g[C.level_key("mvar", "s64j1", size)].any()
        assert not R.variance_map(maps["s64j1"][0], 1, size).any()


def test_out_of_bounds_coordinate_zeroes_the_sample(maps):
    """56 -> 28 and 28 -> 14: zoom * (m - 1) rounds one ulp above n - 1, scipy's sample there is cval = 0 (not
    the edge value), and the goldens hold it: dropping the rule from the restatement is rejected."""
    g = npz(C.GOLDENS)
    for name, n, T in (("s224n3", 56, 28), ("s225", 28, 14)):
        assert ((n - 1) / (T - 1)) * (T - 1) > n - 1
        H, J = C.LEVEL_CASES[name][:2]
        m = maps[name][0]
        block = [b for b in R.diagonal(m, J)[:J] if b.shape[0] == n][0]
        z = R.zoom_block(block, T)
        assert not z[-1].any() and not z[:, -1].any() and z[:-1, :-1].all()
        clamped = R.variance_map(m, J, "minimal", coord=lambda o, n_, m_: np.minimum(((n_ - 1) / (m_ - 1)) * o, n_ - 1))
        want = g[C.level_key("vmap", name, "minimal")][0]
        assert np.abs(clamped - want).max() > 1e3 * R.var_atol(J, m)


def test_other_coordinate_formula_breaks_the_bar_where_scipy_overshoots(maps):
    """(o * (n - 1)) / (m - 1) instead of scipy's zoom * o. Where both stay inside [0, n - 1] the two differ by
    an ulp of the coordinate, i.e. about n u |dv| in the value: at s100 (50 / 25 / 13) that is 0.02 of var_atol
    and stays inside the bar, so that case pins the block geometry and the non-dyadic weights, not the rounding
    of the coordinate. At s225 "minimal" (28 -> 14) scipy's product rounds above n - 1 and its sample is 0,
    the other formula lands on n - 1 exactly and returns the edge value: far outside the bar."""
    g = npz(C.GOLDENS)
    other = lambda o, n_, m_: (o * (n_ - 1)) / (m_ - 1)   # noqa: E731
    ratio = {}
    for name, size in (("s100", "maximal"), ("s100", "minimal"), ("s225", "minimal")):
        H, J = C.LEVEL_CASES[name][:2]
        m = maps[name][0]
        got = R.variance_map(m, J, size, coord=other)
        ratio[name, size] = np.abs(got - g[C.level_key("vmap", name, size)][0]).max() / R.var_atol(J, m)
    assert ratio["s225", "minimal"] > 1e3, ratio
    assert 0 < max(ratio["s100", "maximal"], ratio["s100", "minimal"]) < 1.0, ratio


def test_ranking(maps):
    g = npz(C.GOLDENS)
    for name in C.RANK_CASES:
        J = C.LEVEL_CASES[name][1]
        for size in C.SIZES:
            r = R.rank(maps[name], J, size)
            assert [x["image_index"] for x in r] == list(g[C.level_key("rank", name, size)])
            assert sorted(x["mean_pixelwise_variance"] for x in r) == sorted(g[C.level_key("mvar", name, size)])


def test_iou_counts_and_means_are_exact():
    g = npz(C.GOLDENS)
    cases = {k: C.make_iou_maps(*v) for k, v in C.iou_cases().items()}
    cases[C.IOU_TWINS[0]] = C.make_twins(C.IOU_TWINS[1])
    for name, m in cases.items():
        inter, uni = R.pair_counts(m, C.PERCENTAGES)
        assert np.array_equal(inter, g["inter_" + name]) and np.array_equal(uni, g["uni_" + name]), name
        assert np.array_equal(R.mean_iou(inter, uni), g["miou_" + name]), name
    assert np.array_equal(g["miou_" + C.IOU_TWINS[0]], np.ones(len(C.PERCENTAGES)))
    # p = 0 indexes -1, the minimum: everything is selected; the maps are tied at every threshold
    assert (g["inter_m2_l20"][C.PERCENTAGES.index(0.0)] == 20).all()
    assert (g["uni_m5_l1000"] > np.array([int(1000 * p) for p in C.PERCENTAGES])[:, None]).any()


# ---- host-only functions of wam_amd.utils

def test_get_diagonal_views_and_order():
    m = C.make_maps(30, 1, 5)[0]
    d = utils.get_diagonal(m, 3)
    assert list(d) == ["level_0", "level_1", "level_2", "approx"]
    assert [v.shape for v in d.values()] == [(15, 15), (8, 8), (4, 4), (3, 3)]
    for got, want in zip(d.values(), R.diagonal(m, 3)):
        assert np.shares_memory(got, m) and np.array_equal(got, want)
    with pytest.raises(AssertionError, match="grad_wam must be square"):
        utils.get_diagonal(np.zeros((4, 6)), 1)


def test_iou_of_masks():
    a = np.array([True, True, False, False])
    b = np.array([True, False, True, False])
    assert utils.iou(a, b) == 1 / 3
    assert utils.iou(np.zeros(5, bool), np.zeros(5, bool)) == 0


def test_get_mean_across_images():
    rs = np.random.RandomState(3)
    all_grads = [[rs.uniform(size=4) for _ in range(5)], [rs.uniform(size=4) for _ in range(2)]]
    got = utils.get_mean_across_images(all_grads)
    assert len(got) == 2
    for g_, grads in zip(got, all_grads):
        assert np.array_equal(g_, np.mean(np.array(grads), axis=0))


def test_errors_are_raised_before_anything_is_launched():
    """The reference's exception types, from host-side checks: none of these needs a device."""
    with pytest.raises(AssertionError, match="grad_wam must be square"):
        utils.get_mean_pixelwise_variance(np.zeros((8, 6)), 2)
    with pytest.raises(ValueError, match="size must be 'maximal' or 'minimal'"):
        utils.get_mean_pixelwise_variance(np.zeros((8, 8)), 2, size="median")
    with pytest.raises(ZeroDivisionError):
        utils.get_mean_pixelwise_variance(np.zeros((4, 4)), 4)
    with pytest.raises(ZeroDivisionError):
        R.zoom_length(0, 2)


def test_no_images_is_an_empty_result():
    assert utils.rank_images([], 3) == [] and utils.rank_images(np.zeros((0, 8, 8)), 3, size="minimal") == []
    assert utils.level_shares(np.zeros((0, 8, 8)), 3).shape == (0, 4)


def test_zoom_lengths_match_the_restatement():
    for H, J in [(32, 3), (30, 3), (8, 3), (7, 2), (100, 3), (225, 4), (64, 1), (224, 3)]:
        for size in C.SIZES:
            T, lens = utils._zoom_lengths(H, J, size)
            assert T == R.target_side(H, J, size)
            assert lens == [R.zoom_length(n, T) for n in R.detail_sides(H, J)]


# ---- the C entry points' host-side answers (no launch is reached)

def test_level_stats_host_checks():
    lib = _lib.lib
    assert lib.wam_level_stats_ws_bytes(1, 224, 3, 0) == 8 * 4 * 25            # 112^2 / 512 -> 25 parts per block
    assert lib.wam_level_stats_ws_bytes(2, 224, 3, 112) == 8 * 2 * (4 * 25 + 196)
    assert lib.wam_level_stats_ws_bytes(1, 8, 3, 1) == 8 * (4 + 1)
    assert lib.wam_level_stats_ws_bytes(1, 8, 17, 1) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lens = (ctypes.c_int32 * 3)(4, 3, 4)   # a level shorter than T = 4: the reference's np.stack fails
    assert lib.wam_level_stats(1, 8, 3, p, 4, lens, None, p, None, p, 512, None) == 2      # WAM_ERR_SHAPE
    assert lib.wam_level_stats(1, 8, 3, None, 4, lens, None, p, None, p, 512, None) == 1   # WAM_ERR_INVALID_ARG
    assert lib.wam_level_stats(1, 8, 17, p, 0, None, p, None, None, p, 512, None) == 1
    assert lib.wam_level_stats(1, 4, 4, p, 1, (ctypes.c_int32 * 4)(1, 1, 1, 1), None, p, None, p, 512, None) == 1
    # blocks of 2^31 elements or more: 32-bit index arithmetic in the kernels. With levels == 0 the one block is the map
    assert lib.wam_level_stats(1, 65536, 0, p, 0, None, p, None, None, p, 512, None) == 3   # WAM_ERR_UNSUPPORTED
    assert lib.wam_level_stats(1, 92682, 1, p, 0, None, p, None, None, p, 1024, None) == 3


def test_mask_iou_host_checks():
    lib = _lib.lib
    assert utils._iou_limits() == (16, 16)   # the bounds the header documents; the chunks are sized by the query
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.wam_mask_iou(17, 1, 4, p, p, p, p, None) == 3   # WAM_ERR_UNSUPPORTED: the caller chunks
    assert lib.wam_mask_iou(2, 17, 4, p, p, p, p, None) == 3
    assert lib.wam_mask_iou(1, 1, 4, p, p, p, p, None) == 1
    assert lib.wam_mask_iou(2, 1, 4, None, p, p, p, None) == 1
