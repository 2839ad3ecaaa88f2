"""Eval3DWAM as far as it goes without a device: the evaluator's host position table against the cube
packing of oracle.wam_ref.refactor_3d, the restatement of tests/eval3d_ref.py against itself, and the
route / workspace queries of wam_waverec_ranked on host-only plans. CPU only."""
import ctypes

import numpy as np
import pytest

from oracle import dwt
from tests import eval3d_ref as R
from tests.test_wavedec_adjoint_host import host_plan


def band_shapes(S, J, wavelet="haar"):
    return [b.shape for b in R.flat_bands(dwt.wavedec3(np.zeros((S, S, S)), wavelet, J, "symmetric"))]


@pytest.mark.parametrize("S,J", [(8, 1), (8, 2), (16, 3)])
def test_host_pos_table_inverts_refactor_3d(S, J):
    """pos[k] is the cube voxel refactor_3d writes coefficient k to, and a permutation of range(S^3)."""
    from wam_amd.evaluation3d import cube_pos_table
    pos = cube_pos_table(S, J, band_shapes(S, J))
    assert pos.dtype == np.int32 and pos.shape == (S ** 3,)
    assert np.array_equal(np.sort(pos), np.arange(S ** 3))
    assert np.array_equal(pos, R.coeff_voxels(S, J))
    # the approximation sits in the cube's corner, the finest 'ddd' band in the far octant
    assert pos[0] == 0 and pos[-1] == S ** 3 - 1


def test_host_pos_table_refuses_a_cube_that_is_no_bijection():
    """Haar J=2 at 10^3: bands of 3^3 and 5^3, 1091 coefficients for 1000 cube voxels."""
    from wam_amd.evaluation3d import cube_pos_table
    shapes = band_shapes(10, 2)
    assert sum(int(np.prod(s)) for s in shapes) == 1091
    with pytest.raises(ValueError, match="bijection onto the coefficients.*1091 coefficients for 1000"):
        cube_pos_table(10, 2, shapes)
    with pytest.raises(ValueError, match="bijection"):        # db2 at 8^3: longer bands
        cube_pos_table(8, 1, band_shapes(8, 1, "db2"))


def test_thresholds_and_stable_order():
    assert R.mask_thr(4, 512) == [0, 128, 256, 384, 512]
    assert R.mask_thr(17, 512) == [0] + [30 * m for m in range(1, 17)] + [512]     # the forced-full last mask
    assert R.mask_thr(2, 5) == [0, 2, 5]
    # ties: the later index of equal values comes first (a stable ascending sort, reversed)
    assert R.descending_order(np.array([1.0, 3.0, 1.0, 3.0])).tolist() == [3, 1, 2, 0]


@pytest.mark.parametrize("J", [1, 2])
def test_restatement_end_points(J):
    """Insertion's last mask and deletion's first reconstruct the volume, the other end is all zero,
    and mask m of insertion keeps exactly thr(m) coefficients."""
    rng = np.random.RandomState(J)
    x = rng.standard_normal((8, 8, 8))
    cube = rng.standard_normal((8, 8, 8))
    n_iter = 5
    ins = R.masked_sets(x, cube, "insertion", n_iter, J)
    dele = R.masked_sets(x, cube, "deletion", n_iter, J)
    assert np.abs(dwt.waverec3(ins[-1], "haar") - x).max() < 1e-12
    assert np.abs(dwt.waverec3(dele[0], "haar") - x).max() < 1e-12
    assert np.abs(dwt.waverec3(ins[0], "haar")).max() == 0 and np.abs(dwt.waverec3(dele[-1], "haar")).max() == 0
    for m, thr in enumerate(R.mask_thr(n_iter, 512)):
        kept = sum(int(np.count_nonzero(b)) for b in R.flat_bands(ins[m]))
        assert kept == thr
    # the voxels mask 1 keeps are the thr(1) largest cube values, carried through the packing
    vox = R.coeff_voxels(8, J)
    kept1 = np.concatenate([b.reshape(-1) != 0 for b in R.flat_bands(ins[1])])
    assert set(vox[kept1]) == set(np.argsort(cube.reshape(-1))[::-1][:R.mask_thr(n_iter, 512)[1]])


def test_route_and_workspace_queries_on_host_plans():
    """wam_waverec_ranked_route: 1 for 3D Haar, J <= 2, divisible sizes; 0 for every other 3D plan;
    negative for a 2D plan. The workspace is route 0's alone."""
    from wam_amd import _lib
    lib = _lib.lib
    cases = [((3, (8, 8, 8), 1, "haar", "symmetric", 0), 1), ((3, (8, 12, 16), 2, "haar", "symmetric", 0), 1),
             ((3, (8, 8, 8), 2, "haar", "symmetric", 1), 0),          # WAM_PLAN_GENERIC
             ((3, (16, 16, 16), 3, "haar", "symmetric", 0), 0), ((3, (10, 10, 10), 2, "haar", "symmetric", 0), 0),
             ((3, (12, 12, 12), 2, "db2", "symmetric", 0), 0)]
    for args, want in cases:
        h = host_plan(*args)
        try:
            assert lib.wam_waverec_ranked_route(h) == want, args
            K = lib.wam_plan_coeff_numel(h)
            assert lib.wam_waverec_ranked_workspace_bytes(h, 2, 5, 1) == 0
            w0 = lib.wam_waverec_ranked_workspace_bytes(h, 2, 5, 0)
            assert w0 >= 2 * 6 * K * 4 + lib.wam_plan_workspace_bytes(h, 12)
            assert lib.wam_waverec_ranked_workspace_bytes(h, 2, 5, -1) == (0 if want else w0)
            assert lib.wam_waverec_ranked_workspace_bytes(h, 2, 0, 0) == 0       # n_iter < 1
            # a host-only plan is refused by the compute entry
            buf = (ctypes.c_float * 8)()
            p = ctypes.cast(buf, ctypes.c_void_p)
            assert lib.wam_waverec_ranked(h, 1, p, p, 8, p, 2, 4, 0, -1, p, p, None) == 1
        finally:
            lib.wam_plan_destroy(h)
    h = host_plan(2, (32, 32), 2, "haar", "symmetric")
    try:
        assert lib.wam_waverec_ranked_route(h) < 0
        assert lib.wam_waverec_ranked_workspace_bytes(h, 2, 5, 0) == 0
    finally:
        lib.wam_plan_destroy(h)
    assert lib.wam_waverec_ranked_route(None) < 0
    assert lib.wam_waverec_ranked(None, 1, None, None, 1, None, 1, 1, 0, -1, None, None, None) == 1
