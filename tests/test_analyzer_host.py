"""WAMAnalyzer2D's host-side checks: everything wam_threshold_mask_coeffs cannot check itself (it is handed
pointers, not lengths) is refused in Python before anything is launched. These tests run without a device:
had the code reached a launch, or even a device allocation, they would fail with another error."""
import numpy as np
import pytest
import torch

from wam_amd import analysis as A


def bare_analyzer(n_maps, size=32):
    """An analyzer without a model or a device: only what the checks read."""
    an = object.__new__(A.WAMAnalyzer2D)
    an.grad_wams = np.random.RandomState(0).uniform(size=(n_maps, size, size))
    an.J, an.wavelet, an.normalize, an.eval_batch = 2, "haar", "reference", 520
    an.model, an.device = None, None   # touching the device property would raise something else
    an.insertion_quantile, an.deletion_quantile = [], []
    return an


def test_match_counts():
    maps = np.zeros((4, 8, 8))
    assert A.match_counts(4, maps) == 4
    assert A.match_counts(2, maps) == 2                           # surplus maps stay unused, as in the reference
    assert A.match_counts(8, maps, reference_zip=True) == 4       # isolate_scales zips: the shorter one
    assert A.match_counts(2, maps, reference_zip=True) == 2
    with pytest.raises(IndexError, match="4 maps for 8 images"):
        A.match_counts(8, maps)


def test_fewer_cached_maps_than_images_is_an_index_error_before_any_device_work():
    """grad_wams cached from a 4-image call, then an 8-image batch: the reference's IndexError, raised on
    the host (there is no device here to launch on)."""
    an = bare_analyzer(4)
    x = torch.rand(8, 3, 32, 32)
    with pytest.raises(IndexError, match="4 maps for 8 images"):
        an.isolate_necessary_components(x, [0] * 8, [0.9, 0.5], mode="insertion")
    assert an.insertion_quantile == []


class StubPlan:
    coeff_numel = 1024
    rec_shape = (32, 32)

    def wavedec(self, x):
        raise AssertionError("reached the device")


@pytest.mark.parametrize("what", ["map rows", "map length", "threshold rows", "threshold range", "positions", "dtype",
                                  "level edges", "coefficients"])
def test_masked_reconstructions_checks_every_length(what):
    N, size, Q = 3, 32, 5
    planes = torch.zeros(N, 3, size, size)
    maps = torch.zeros(N, size * size, dtype=torch.float64)
    thr = torch.zeros(N, Q, dtype=torch.float64)
    pos = torch.zeros(StubPlan.coeff_numel, dtype=torch.int32)
    kw = {}
    if what == "map rows":
        maps = maps[:2]
    elif what == "map length":
        maps = maps[:, :-1].contiguous()
    elif what == "threshold rows":
        thr = thr[:2]
    elif what == "threshold range":
        kw = dict(q0=3, n_thr=3)
    elif what == "positions":
        pos = pos[:-4]
    elif what == "dtype":
        maps = maps.float()
    elif what == "level edges":
        kw = dict(level=True, strict=True, edges=[32, 16])
    elif what == "coefficients":
        kw = dict(coeffs=torch.zeros(2 * 3 * StubPlan.coeff_numel))
    with pytest.raises(ValueError):
        A.masked_reconstructions(StubPlan(), pos, size, planes, maps, thr, **kw)
