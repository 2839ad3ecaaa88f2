"""The wavedec adjoint's C entry points, as far as they go without a device: the symbols, the argument
checks, the workspace size and the route query on host-only plans (wam_plan_create_host)."""
import ctypes

import pytest

from wam_amd import _lib, filters

lib = _lib.lib


def host_plan(ndim, shape, levels, wavelet, mode, flags=0):
    w = filters.get_wavelet(wavelet)
    L = len(w.dec_lo)
    arr = lambda v: (ctypes.c_double * L)(*v)
    h = ctypes.c_void_p()
    rc = lib.wam_plan_create_host(ctypes.byref(h), ndim, (ctypes.c_int64 * ndim)(*shape), levels, arr(w.dec_lo),
                                  arr(w.dec_hi), arr(w.rec_lo), arr(w.rec_hi), L, filters.mode_id(mode), flags)
    assert rc == 0
    return h


def routes(h, levels):
    return [lib.wam_plan_wavedec_adjoint_route(h, l) for l in range(levels)]


def test_symbols():
    for name in ("wam_wavedec_adjoint", "wam_wavedec_adjoint_workspace_bytes", "wam_plan_wavedec_adjoint_route"):
        assert hasattr(lib, name) and name in _lib._SIGS


def test_null_arguments():
    assert lib.wam_wavedec_adjoint(None, 1, None, None, None, None) == 1
    assert lib.wam_wavedec_adjoint_workspace_bytes(None, 1) < 0
    assert lib.wam_plan_wavedec_adjoint_route(None, 0) < 0


def test_host_plan_is_refused_by_the_compute_entry():
    h = host_plan(2, (32, 32), 2, "db4", "reflect")
    try:
        buf = (ctypes.c_float * 8)()
        p = ctypes.cast(buf, ctypes.c_void_p)
        # non-NULL pointers everywhere: only the missing device side of the plan is left to refuse
        assert lib.wam_wavedec_adjoint(h, 1, p, p, p, None) == 1
        assert lib.wam_wavedec_adjoint(h, -1, p, p, p, None) == 1
    finally:
        lib.wam_plan_destroy(h)


@pytest.mark.parametrize("ndim,shape,levels,wavelet", [(1, (4001,), 5, "db6"), (2, (224, 224), 3, "db4"),
                                                       (2, (9, 11), 2, "db4"), (3, (17, 18, 19), 2, "db2")])
def test_workspace(ndim, shape, levels, wavelet):
    h = host_plan(ndim, shape, levels, wavelet, "reflect")
    try:
        assert lib.wam_wavedec_adjoint_workspace_bytes(h, -1) < 0
        b1, b4 = (lib.wam_wavedec_adjoint_workspace_bytes(h, b) for b in (1, 4))
        assert 0 < b1 <= b4
        for b in (0, 1, 4):  # the transforms' shared workspace always suffices
            assert lib.wam_wavedec_adjoint_workspace_bytes(h, b) <= lib.wam_plan_workspace_bytes(h, b)
    finally:
        lib.wam_plan_destroy(h)


def test_routes():
    AXIS, FOLD = 0, 1
    cases = [
        ((2, (224, 224), 3, "db4", "reflect", 0), [FOLD] * 3),
        ((2, (224, 224), 3, "db4", "reflect", 1), [AXIS] * 3),          # WAM_PLAN_GENERIC
        ((2, (224, 224), 3, "db4", "zero", 0), [FOLD] * 3),
        ((1, (4001,), 5, "db6", "reflect", 0), [AXIS] * 5),
        ((3, (17, 18, 19), 2, "db2", "reflect", 0), [AXIS] * 2),
        # db4: p = 6; level inputs (20, 23) -> (13, 15) -> (10, 11) -> (8, 9) -> (7, 8) -> (7, 7) -> (7, 7)
        ((2, (20, 23), 2, "db4", "symmetric", 0), [FOLD, FOLD]),
        # (9, 11) -> (8, 9) -> ...: every level above the pad; (6, 30) has its first axis at n == p
        ((2, (6, 30), 2, "db4", "reflect", 0), [AXIS, AXIS]),
        ((2, (7, 30), 1, "db4", "reflect", 0), [FOLD]),
        # sym8: p = 14; (20, 23) -> (17, 19) -> (16, 17); (30, 14): n == p on the second axis
        ((2, (30, 14), 1, "sym8", "reflect", 0), [AXIS]),
        ((2, (64, 64), 2, "db11", "reflect", 0), [AXIS, AXIS]),         # 22 taps: beyond the fused kernels
    ]
    for (ndim, shape, levels, wavelet, mode, flags), want in cases:
        h = host_plan(ndim, shape, levels, wavelet, mode, flags)
        try:
            assert routes(h, levels) == want, (shape, wavelet, mode, flags)
            assert lib.wam_plan_wavedec_adjoint_route(h, levels) < 0
            assert lib.wam_plan_wavedec_adjoint_route(h, -1) < 0
        finally:
            lib.wam_plan_destroy(h)
