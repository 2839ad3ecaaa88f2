"""Eval3DWAM.mu_fidelity as far as it goes without a device: the 3D cell map against scipy's zoom of actual
float masks, the restatement of tests/eval3d_mu_ref.py against itself, three 1-D reference passes against
scipy.ndimage.gaussian_filter in bits, and the route / workspace queries of wam_waverec_cells on host-only
plans. CPU only."""
import ctypes
import random

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

from tests import eval3d_mu_ref as M
from tests import evalkern_ref as K
from tests.test_wavedec_adjoint_host import host_plan

INVALID, UNSUPPORTED = 1, 3


@pytest.mark.parametrize("g,S", [(4, 8), (3, 8), (4, 16), (8, 16), (5, 12), (1, 8), (8, 8)])
def test_cell_map_is_the_zoom_of_float_masks(g, S):
    from wam_amd.evalcore import zoom_cell_map3
    cell = zoom_cell_map3(g, S)
    assert cell.shape == (S, S, S) and cell.dtype == np.int64
    assert np.array_equal(np.unique(cell), np.arange(g ** 3))
    masks = np.random.RandomState(g + S).standard_normal((3, g, g, g)).astype(np.float32)
    up = M.upsample(masks, S)
    assert up.dtype == np.float32
    K.assert_bits(masks.reshape(3, -1)[:, cell.reshape(-1)].reshape(up.shape), up, "cell map %d -> %d" % (g, S))


def test_cell_map_refuses_a_grid_with_empty_cells():
    from wam_amd.evalcore import zoom_cell_map3
    with pytest.raises(ValueError, match="non-empty"):
        zoom_cell_map3(9, 8)
    with pytest.raises(ValueError):
        zoom_cell_map3(0, 8)


@pytest.mark.parametrize("J", [1, 2])
def test_all_ones_masks_reproduce_the_volume(J):
    x = np.random.RandomState(J).standard_normal((8, 8, 8))
    rec = M.masked_recs(x, np.ones((2, 4, 4, 4), np.float32), J)
    assert rec.shape == (2, 8, 8, 8) and np.abs(rec - x).max() < 1e-12
    # a mask of zeros removes everything
    assert np.abs(M.masked_recs(x, np.zeros((1, 4, 4, 4), np.float32), J)).max() == 0


@pytest.mark.parametrize("shape,sigma", [((5, 7, 9), 2), ((8, 8, 8), 2), ((16, 12, 8), 2), ((3, 1, 9), 2),
                                         ((6, 10, 4), 1), ((4, 6, 5), 8)])
def test_three_passes_are_scipy_gaussian_filter_in_bits(shape, sigma):
    x = np.random.RandomState(sum(shape)).standard_normal(shape) * 3 + 0.5
    w, r = K.gaussian_weights(sigma)
    got = x
    for axis in (0, 1, 2):
        got = K.gauss_pass(got, w, r, axis)
    K.assert_bits(got, gaussian_filter(x, sigma), "three passes %s sigma %s" % (shape, sigma))


def test_route_and_workspace_queries_on_host_plans():
    from wam_amd import _lib
    lib = _lib.lib
    cases = [((3, (8, 8, 8), 1, "haar", "symmetric", 0), True), ((3, (8, 12, 16), 2, "haar", "symmetric", 0), True),
             ((3, (8, 8, 8), 2, "haar", "symmetric", 1), False),          # WAM_PLAN_GENERIC
             ((3, (16, 16, 16), 3, "haar", "symmetric", 0), False), ((3, (10, 10, 10), 2, "haar", "symmetric", 0), False),
             ((3, (12, 12, 12), 2, "db2", "symmetric", 0), False)]
    for args, served in cases:
        h = host_plan(*args)
        try:
            own = lib.wam_waverec_cells_route(h)
            assert own in (0, 1) and (served or own == 0), args
            Kc = lib.wam_plan_coeff_numel(h)
            sets, n_masks = 3, 17
            assert lib.wam_waverec_cells_workspace_bytes(h, sets, n_masks, 1) == 0
            w0 = lib.wam_waverec_cells_workspace_bytes(h, sets, n_masks, 0)
            assert w0 == (sets * n_masks * Kc * 4 + 15) // 16 * 16 + lib.wam_plan_workspace_bytes(h, sets * n_masks)
            assert lib.wam_waverec_cells_workspace_bytes(h, sets, n_masks, -1) == (0 if own else w0)
            for bad in ((-1, n_masks, 0), (sets, 0, 0), (sets, n_masks, 2), (sets, n_masks, -2)):
                assert lib.wam_waverec_cells_workspace_bytes(h, *bad) == 0
            # a host-only plan is refused by the compute entry
            buf = (ctypes.c_float * 8)()
            p = ctypes.cast(buf, ctypes.c_void_p)
            assert lib.wam_waverec_cells(h, 1, p, p, 2, 8, p, -1, p, p, None) == INVALID
        finally:
            lib.wam_plan_destroy(h)
    h = host_plan(2, (32, 32), 2, "haar", "symmetric")
    try:
        assert lib.wam_waverec_cells_route(h) == -UNSUPPORTED
        assert lib.wam_waverec_cells_workspace_bytes(h, 2, 5, 0) == 0
    finally:
        lib.wam_plan_destroy(h)
    assert lib.wam_waverec_cells_route(None) == -INVALID
    assert lib.wam_waverec_cells_workspace_bytes(None, 2, 5, 0) == 0
    assert lib.wam_waverec_cells(None, 1, None, None, 1, 1, None, -1, None, None, None) == INVALID
    assert lib.wam_gaussian_filter3d(1, 4, 4, 4, None, 0, None, None, None, None) == INVALID


def test_restatement_draws_and_leaves_the_global_random_state_alone():
    import testmodels
    import torch
    model = testmodels.TinyVoxel()
    x = torch.rand(2, 1, 8, 8, 8, generator=torch.Generator().manual_seed(8)).numpy()
    gw = np.random.RandomState(3).uniform(size=(2, 8, 8, 8)).astype(np.float32)
    random.seed(5)
    np.random.seed(5)
    st, nst = random.getstate(), np.random.get_state()
    a = M.mu_fidelity(model, x, [1, 3], gw, 2, 4, 16, 13)
    assert random.getstate() == st
    now = np.random.get_state()
    assert now[0] == nst[0] and np.array_equal(now[1], nst[1]) and now[2:] == nst[2:]
    b = M.mu_fidelity(model, x, [1, 3], gw, 2, 4, 16, 13)
    for da, db in zip(a, b):                                           # fresh generators at every call
        assert da["mu"] == db["mu"] and da["subsets"] == db["subsets"] and np.array_equal(da["source"], db["source"])
    # the protocol: volume 1's draws follow volume 0's in both streams
    subsets, sources = M.draws(42, 2, 4, 16, 13)
    assert subsets[1] == a[1]["subsets"] and subsets[0] != subsets[1] and not np.array_equal(sources[0], sources[1])
    for d in a:
        assert -1.0 <= d["mu"] <= 1.0 and d["baseline_index"] == int(np.argmin(d["baseline_probs"]))
        assert all(len(s) == 13 and len(set(s)) == 13 and max(s) < 64 for s in d["subsets"])
        assert d["source"].dtype == np.float32 and d["source"].shape == (16, 4, 4, 4)
        # handing the index over changes nothing when it is the restatement's own
    c = M.mu_fidelity(model, x, [1, 3], gw, 2, 4, 16, 13, baseline_index=[d["baseline_index"] for d in a])
    assert [d["mu"] for d in c] == [d["mu"] for d in a]
