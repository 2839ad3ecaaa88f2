"""tests/moments_ref.py (the float64 restatement the GPU tests of 'smooth_sq' / 'vargrad' compare
against) pinned on the CPU: its sample-order sums equal numpy's own mean of squares and variance of
the stacked per-sample maps to 1e-12, and the 2D inputs carry a variance large enough to test
against -- the 2e-4 / 4e-4 bars of tests/test_gpu_moments.py are meant to stay under 1 % of it."""
import numpy as np
import pytest

from tests import moments_ref as M


def _check(mo, v):
    v = np.asarray(v, dtype=np.float64)
    assert np.abs(mo["smooth_sq"] - np.mean(v ** 2, axis=0)).max() <= 1e-12 * max(1.0, float((v ** 2).max()))
    assert np.abs(mo["vargrad"] - np.var(v, axis=0)).max() <= 1e-12 * max(1.0, float((v ** 2).max()))
    assert np.abs(mo["mean"] - np.mean(v, axis=0)).max() <= 1e-12 * max(1.0, float(np.abs(v).max()))
    assert (mo["vargrad"] >= 0).all()


@pytest.mark.parametrize("name,vmax", [("haar_J2_32", 0.048), ("db4_J3_64", 0.140)])
def test_moments_ref_2d(name, vmax):
    """TinySmooth2D, torch.rand inputs (seed 1), labels [1, 3], stdev_spread 0.25, 6 samples, native
    frame. The variance's maximum is at least 0.04 (measured: 0.048 haar J=2 at 32^2, 0.140 db4 J=3 at
    64^2), so the GPU bars of 2e-4 / 4e-4 are under 1 % of it; the map values lie in [0, 1]."""
    r = M.ref_2d(name)
    v = r["maps"]
    assert v.shape == (M.N_SAMPLES, 2, M.CASES_2D[name]["size"], M.CASES_2D[name]["size"])
    assert v.min() >= 0.0 and v.max() <= 1.0
    _check(r, v)
    got = float(r["vargrad"].max())
    print("[moments_ref] %s: max vargrad %.4f, max smooth_sq %.4f" % (name, got, float(r["smooth_sq"].max())))
    assert got >= 0.04
    assert abs(got - vmax) < 0.002


def test_moments_ref_n1_is_zero_and_nan_propagates():
    v = np.random.RandomState(0).uniform(0, 1, (1, 7)).astype(np.float32)
    assert not M.moments(list(v))["vargrad"].any()
    w = np.random.RandomState(1).uniform(0, 1, (3, 7))
    w[1, 2] = np.nan
    mo = M.moments(list(w))
    for k in ("mean", "smooth_sq", "vargrad"):
        assert np.array_equal(np.isnan(mo[k]), np.arange(7) == 2)


def test_moments_ref_1d_3d():
    """The 1D (TinyAudio, db6 J=2, 4096 samples) and 3D (TinyVoxel, Haar J=2 at 16^3, spread 0.05)
    restatements against numpy on the stacked per-sample gradients."""
    r1 = M.ref_1d()
    flat = lambda t: np.concatenate([t[0].ravel()] + [c.ravel() for c in t[1]])
    _check({k: flat(r1[k]) for k in ("mean", "smooth_sq", "vargrad")}, r1["maps"])
    assert r1["mean"][0].shape[0] == 2 and len(r1["mean"][1]) == 3
    r3 = M.ref_3d()
    _check(r3, r3["maps"])
    assert r3["maps"].shape == (M.N_SAMPLES, 2, 16, 16, 16) and r3["vargrad"].max() > 0
