"""tests/wavedec_adjoint_ref.py (the formula of the wavedec adjoint, float64 numpy) against autograd through
oracle.ptwt_torch.wavedec* in float64, every boundary mode, 1D-3D, lengths down to below the pad. Also
records each case's d32: how far the oracle's own float32 autograd lies from its float64 run, the scale
of the GPU tests' bars."""
import numpy as np
import pytest
import torch

from oracle import dwt as D

from tests import wavedec_adjoint_ref as R


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_formula_equals_oracle_autograd(case, mode):
    ndim, wavelet, shape, levels = case
    dec_lo, dec_hi, _, _ = D.filter_bank(wavelet)
    x, grads = R.case_inputs(case)
    ref = R.oracle_gradient(x, grads, wavelet, mode, levels, torch.float64)
    got = R.wavedec_adjoint(grads, shape, dec_lo, dec_hi, mode, levels)
    assert got.shape == ref.shape == x.shape
    scale = max(1.0, np.abs(ref).max())
    assert np.abs(got - ref).max() <= 1e-12 * scale
    d32 = np.abs(R.oracle_gradient(x, grads, wavelet, mode, levels, torch.float32) - ref).max()
    print("%s %s d32=%.3g d32/max|ref|=%.3g" % (R.case_id(case), mode, d32, d32 / np.abs(ref).max()))
    # float32 autograd of the same graph: a few ulps (6e-8) of the result per accumulated term, a term
    # per tap, axis and level
    assert d32 <= 1e-5 * scale


@pytest.mark.parametrize("mode", R.MODES)
def test_dot_product_identity(mode):
    """<wavedec(x), c> == <x, adjoint(c)> with the oracle's float64 forward."""
    from oracle import ptwt_torch as P
    case = (2, "db4", (9, 11), 2)
    x, grads = R.case_inputs(case, batch=3, seed=5)
    dec_lo, dec_hi, _, _ = D.filter_bank("db4")
    bands = R.oracle_bands(P.wavedec2(torch.tensor(x), "db4", mode=mode, level=2), 2)
    lhs = sum(float((b.numpy() * g).sum()) for b, g in zip(bands, grads))
    rhs = float((x * R.wavedec_adjoint(grads, (9, 11), dec_lo, dec_hi, mode, 2)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


@pytest.mark.parametrize("wavelet", ["haar", "db4", "sym8"])
@pytest.mark.parametrize("shape", [(8, 8), (9, 11), (20, 23)])
def test_zero_mode_orthogonal_equals_cropped_waverec(wavelet, shape):
    """Orthogonal wavelet, zero mode: the adjoint is waverec of the same coefficients cropped to the shape."""
    from oracle import ptwt_torch as P
    case = (2, wavelet, shape, 2)
    _, grads = R.case_inputs(case)
    dec_lo, dec_hi, _, _ = D.filter_bank(wavelet)
    got = R.wavedec_adjoint(grads, shape, dec_lo, dec_hi, "zero", 2)
    t = [torch.tensor(g) for g in grads]
    rec = P.waverec2([t[0], tuple(t[1:4]), tuple(t[4:7])], wavelet).numpy()
    assert np.abs(got - rec[:, :shape[0], :shape[1]]).max() <= 1e-12 * max(1.0, np.abs(rec).max())
