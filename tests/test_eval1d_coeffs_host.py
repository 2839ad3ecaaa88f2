"""Eval1DWAM(mask_layout="coeffs") as far as it goes without a device: the identity slot map and the
thresholds of the host code against the restatement's running-offset slices (tests/eval1d_ref.py), the
keyword validation, and wam_waverec1_ranked's route query and workspace sizes on host-only plans."""
import ctypes

import numpy as np
import pytest

from oracle import dwt
from tests import eval1d_ref as R
from tests.test_wavedec_adjoint_host import host_plan
from wam_amd import _lib

lib = _lib.lib
INVALID, UNSUPPORTED = 1, 3
# wavelet, J, W, K: the three geometries of tests/test_gpu_eval1d_coeffs.py
GEOMS = [("db6", 3, 4096, 4127), ("db2", 2, 9001, 9006), ("sym4", 4, 8300, 8326)]


def band_lens(wavelet, J, W):
    sizes = dwt.level_sizes(W, len(dwt.filter_bank(wavelet)[0]), J)      # finest first
    return [sizes[-1]] + sizes[::-1]                                      # A_J, D_J, ..., D_1


@pytest.mark.parametrize("wavelet,J,W,K", GEOMS)
def test_identity_slot_map_is_the_running_offset_layout(wavelet, J, W, K):
    from wam_amd.evaluation import coeff_identity_map
    lens = band_lens(wavelet, J, W)
    assert sum(lens) == K
    pos = coeff_identity_map(lens, lens)
    assert pos.dtype == np.int32 and pos.shape == (K,)
    # the restatement's mask slice of band i is columns [start, end) of the K-wide mask: exactly n_i
    # wide (no pad column), and the slots of the band's coefficients in order
    off = np.concatenate([[0], np.cumsum(lens)])
    for i, (start, end) in enumerate(R.band_slices(W, J, lens, "running")):
        assert end - start == lens[i]
        assert np.array_equal(pos[off[i]:off[i + 1]], np.arange(start, end))
    with pytest.raises(ValueError, match="the explainer's bands .* are not the evaluation plan's"):
        coeff_identity_map(lens, lens[:-1] + [lens[-1] + 1])
    with pytest.raises(ValueError):
        coeff_identity_map(lens, lens[1:])


@pytest.mark.parametrize("wavelet,J,W,K", GEOMS)
@pytest.mark.parametrize("n_iter", [2, 4, 7, 64])
def test_thresholds(wavelet, J, W, K, n_iter):
    from wam_amd.evaluation import rank_thresholds
    n_comp, thr = rank_thresholds(n_iter, K)
    assert n_comp == int(K / n_iter) and thr == R.thresholds(n_iter, K)
    assert thr[0] == 0 and thr[-1] == K and len(thr) == n_iter + 1
    assert thr == [R._thr(m, n_iter, n_comp, K) for m in range(n_iter + 1)]     # the C ABI's rule


def test_keyword_validation_touches_no_device():
    from wam_amd.evaluation import Eval1DWAM
    for bad in ("mosaic", "pywt", None, ""):
        with pytest.raises(ValueError, match="mask_layout must be 'reference' or 'coeffs', got"):
            Eval1DWAM(object(), wavelet="db6", J=3, mask_layout=bad)


def test_symbols_and_null_plans():
    for name in ("wam_waverec1_ranked", "wam_waverec1_ranked_workspace_bytes", "wam_waverec1_ranked_route",
                 "wam_peak_divide"):
        assert hasattr(lib, name) and name in _lib._SIGS
    assert lib.wam_waverec1_ranked_route(None) == -INVALID
    assert lib.wam_waverec1_ranked_workspace_bytes(None, 1, 8, 0) == 0
    assert lib.wam_waverec1_ranked(None, 1, None, None, 1, None, 8, 1, 0, -1, None, None, None, None) == INVALID
    assert lib.wam_peak_divide(1, 8, None, None, None, None, 0, None) == INVALID
    for ndim, shape in ((2, (16, 16)), (3, (8, 8, 8))):
        h = host_plan(ndim, shape, 1, "haar", "symmetric")
        try:
            assert lib.wam_waverec1_ranked_route(h) == -UNSUPPORTED
            assert lib.wam_waverec1_ranked_workspace_bytes(h, 1, 8, 0) == 0
        finally:
            lib.wam_plan_destroy(h)


@pytest.mark.parametrize("wavelet,W,levels,mode,flags,served", [
    ("db6", 80000, 5, "reflect", 0, True), ("haar", 80000, 5, "reflect", 0, True), ("db10", 9000, 2, "reflect", 0, True),
    ("haar", 8192, 9, "reflect", 0, False), ("haar", 64, 3, "periodic", 0, False), ("haar", 64, 3, "reflect", 1, False)])
def test_route_and_workspace_on_host_plans(wavelet, W, levels, mode, flags, served):
    h = host_plan(1, (W,), levels, wavelet, mode, flags)
    try:
        r = lib.wam_waverec1_ranked_route(h)
        assert r in (0, 1) and (served or r == 0)      # J = 9, periodic and WAM_PLAN_GENERIC: never the fused kernel
        K = lib.wam_plan_coeff_numel(h)
        sets, n_iter = 3, 8
        M = n_iter + 1
        b0 = lib.wam_waverec1_ranked_workspace_bytes(h, sets, n_iter, 0)
        b1 = lib.wam_waverec1_ranked_workspace_bytes(h, sets, n_iter, 1)
        assert b0 == (sets * M * K * 4 + 15) // 16 * 16 + lib.wam_plan_workspace_bytes(h, sets * M)
        assert b1 == (sets * K * 4 + 15) // 16 * 16
        assert lib.wam_waverec1_ranked_workspace_bytes(h, sets, n_iter, -1) == b0 >= b1
        # a host-only plan cannot compute: non-NULL pointers everywhere, only the device side is missing
        buf = (ctypes.c_float * 16)()
        p = ctypes.cast(buf, ctypes.c_void_p)
        assert lib.wam_waverec1_ranked(h, 1, p, p, 4, p, n_iter, 1, 0, 0, p, p, p, None) == INVALID
    finally:
        lib.wam_plan_destroy(h)
