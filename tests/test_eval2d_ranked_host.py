"""wam_waverec2_ranked's C entry points as far as they go without a device: the symbols, the route
query and the workspace sizes on host-only plans (wam_plan_create_host), the refusal of a host-only plan
by the compute entry, and frames.wam_cell_source on plan-shaped host objects."""
import ctypes
import types

import numpy as np
import pytest

from tests.test_wavedec_adjoint_host import host_plan
from wam_amd import _lib

lib = _lib.lib
INVALID, UNSUPPORTED = 1, 3


def test_symbols():
    for name in ("wam_waverec2_ranked", "wam_waverec2_ranked_workspace_bytes", "wam_waverec2_ranked_route"):
        assert hasattr(lib, name) and name in _lib._SIGS


def test_null_and_non_2d_plans():
    assert lib.wam_waverec2_ranked_route(None) == -INVALID
    assert lib.wam_waverec2_ranked_workspace_bytes(None, 1, 3, 8, 0) == 0
    assert lib.wam_waverec2_ranked(None, 1, 3, None, None, 1, None, 8, 1, 0, -1, None, None, None) == INVALID
    for ndim, shape in ((1, (64,)), (3, (8, 8, 8))):
        h = host_plan(ndim, shape, 1, "haar", "symmetric")
        try:
            assert lib.wam_waverec2_ranked_route(h) == -UNSUPPORTED
            assert lib.wam_waverec2_ranked_workspace_bytes(h, 1, 3, 8, 0) == 0
        finally:
            lib.wam_plan_destroy(h)


@pytest.mark.parametrize("wavelet,shape,levels", [("haar", (224, 224), 3), ("db4", (224, 224), 3), ("db6", (24, 24), 2)])
def test_route_and_workspace_on_host_plans(wavelet, shape, levels):
    h = host_plan(2, shape, levels, wavelet, "symmetric")
    try:
        r = lib.wam_waverec2_ranked_route(h)
        assert r in (0, 1) and (wavelet != "db6" or r == 0)         # 12 taps: never the fused kernel
        K = lib.wam_plan_coeff_numel(h)
        images, C, n_iter = 2, 3, 8
        M = n_iter + 1
        b0 = lib.wam_waverec2_ranked_workspace_bytes(h, images, C, n_iter, 0)
        b1 = lib.wam_waverec2_ranked_workspace_bytes(h, images, C, n_iter, 1)
        masked = (images * M * C * K * 4 + 15) // 16 * 16
        assert b0 == masked + lib.wam_plan_workspace_bytes(h, images * M * C)
        assert b1 == (images * K * 4 + 15) // 16 * 16                # the rank table in coefficient order
        assert lib.wam_waverec2_ranked_workspace_bytes(h, images, C, n_iter, -1) == b0 >= b1
        for bad in ((-1, C, n_iter, 0), (1, 0, n_iter, 0), (1, 5, n_iter, 0), (1, C, 0, 0), (1, C, n_iter, 2)):
            assert lib.wam_waverec2_ranked_workspace_bytes(h, *bad) == 0
        # a host-only plan cannot compute: non-NULL pointers everywhere, only the device side is missing
        buf = (ctypes.c_float * 16)()
        p = ctypes.cast(buf, ctypes.c_void_p)
        assert lib.wam_waverec2_ranked(h, 1, C, p, p, 4, p, n_iter, 1, 0, 0, p, p, None) == INVALID
    finally:
        lib.wam_plan_destroy(h)


def fake_plan(shape, bands):
    off = np.concatenate([[0], np.cumsum([h * w for h, w in bands])])
    return types.SimpleNamespace(shape=shape, levels=(len(bands) - 1) // 3, band_shapes=bands,
                                 band_offsets=[int(v) for v in off], coeff_numel=int(off[-1]))


def test_cell_source_haar_is_a_bijection_and_db2_holds_some():
    from wam_amd.frames import wam_cell_source
    haar = fake_plan((32, 32), [(8, 8)] * 4 + [(16, 16)] * 3)
    for method in ("smooth", "integratedgrad"):
        src, shape = wam_cell_source(haar, "native", method)
        assert shape == (32, 32) and src.dtype == np.int64
        assert np.array_equal(np.sort(src.reshape(-1)), np.arange(1024))
    # H (band 4 of the finest level) is drawn top-right, V bottom-left
    src, _ = wam_cell_source(haar, "native", "smooth")
    assert src[0, 16] == haar.band_offsets[4] and src[16, 0] == haar.band_offsets[5]
    db2 = fake_plan((32, 32), [(10, 10)] * 4 + [(17, 17)] * 3)
    src, shape = wam_cell_source(db2, "native", "smooth")
    shown = src[src >= 0]
    assert shape == (32, 32) and np.unique(shown).size == shown.size == 1024 and db2.coeff_numel - shown.size > 0
    with pytest.raises(ValueError):
        wam_cell_source(db2, "legacy", "smooth")                     # the legacy frame is 34 x 34 here
    with pytest.raises(ValueError):
        wam_cell_source(haar, "other", "smooth")
