"""The edges of the DWT launchers' filter-length dispatch (wam_amd/csrc/dispatch.hpp) that the large
suites do not state outright: every listed length of every kernel family launches that family's
kernels, the lengths the rows family leaves out (10, 14, 18) run on the column strips, the 1D
synthesis runs on the persistent kernel up to 8 levels and on k_dwt1_syn above, and a length no
family serves launches nothing. Tiny shapes; the kernels that ran are read from the live timing
records, the statuses at the C ABI.

The expected kernel names, routes and statuses were recorded from the commit before dispatch.hpp
(hand-written switch / macro ladders per launcher), where this file passes unchanged."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import filter_banks as F

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED = 0, 3
GENERIC, NO_ROWS, NO_PLANE = 1, 2, 4
EVEN20 = tuple(range(2, 21, 2))
TO8 = (2, 4, 6, 8)
ROWS = (2, 4, 6, 8, 12, 16, 20)

# family -> (ndim, shape, levels, flags, its lengths, kernels of wavedec / waverec / the maps pass)
FAMILIES = {
    "tile1": (1, (300,), 2, 0, EVEN20, "k_dwt1_ana", "k_dwt1_syn", None),
    "colstrip": (2, (36, 44), 2, NO_ROWS | NO_PLANE, EVEN20, "k_dwt2_ana", "k_dwt2_syn", None),
    "plane": (2, (36, 44), 2, 0, TO8, "k_plane_ana", "k_plane_syn", "k_plane_maps"),
    "rows": (2, (36, 44), 2, NO_PLANE, ROWS, "k_ana_rows", "k_dwt2_syn", "k_adj_maps"),
    "tile3": (3, (9, 10, 11), 1, 0, TO8, "k_dwt3_ana_tile", "k_dwt3_syn_tile", None),
}


@pytest.fixture(scope="module")
def P():
    from wam_amd import plan
    assert torch.cuda.is_available()
    return plan


def launched(P, fn):
    """fn's result and the set of kernel names it launched: template tags dropped, the 1D tile
    kernels' boundary forms (k_dwt1_ana_p, k_dwt1_ana_int) folded to k_dwt1_ana"""
    P.timing_drain()
    P.timing_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        P.timing_enable(False)
    return out, {re.sub(r"^k_dwt1_ana.*", "k_dwt1_ana", r[0].split("<")[0]) for r in P.timing_drain()}


@pytest.mark.parametrize("family,L", [(f, L) for f, v in FAMILIES.items() for L in v[4]])
def test_every_listed_length_launches(P, family, L):
    ndim, shape, J, flags, _, ana, syn, maps = FAMILIES[family]
    p = P.get_plan(ndim, shape, J, F.random_bank(L, L), "reflect", "cuda", flags=flags)
    torch.manual_seed(L)
    B = 3
    x = torch.randn((B,) + shape, device="cuda")
    cf, names = launched(P, lambda: p.wavedec(x))
    assert names == {ana}, (p.routes, names)
    g = torch.randn((B,) + p.rec_shape, device="cuda")
    _, names = launched(P, lambda: p.adjoint(g))
    assert names == {ana}, (p.routes, names)
    rec, names = launched(P, lambda: p.waverec(cf, B, alphas=[0.5, 1.0]))
    # 300 samples are one tile: the persistent 1D synthesis takes it at every length
    assert names == {"k_dwt1_syn_int" if family == "tile1" else syn}, (p.routes, names)
    assert bool(torch.isfinite(cf).all()) and bool(torch.isfinite(rec).all())
    if maps:
        _, names = launched(P, lambda: p.adjoint_maps(g, 1, 1, 3))
        assert names == {maps}, (p.routes, names)
    if family == "colstrip":  # the wavedec adjoint's border kernel shares the column strips' lengths
        _, names = launched(P, lambda: p.wavedec_adjoint(torch.randn_like(cf), B))
        assert names == {"k_dwt2_syn", "k_dwt2_adjoint_border"}, names


@pytest.mark.parametrize("L", [10, 14, 18])
def test_lengths_the_rows_family_leaves_out_take_the_column_strips(P, L):
    p = P.get_plan(2, (36, 44), 2, F.random_bank(L, L), "reflect", "cuda")
    assert p.routes == "ana=none|colstrip,colstrip adj=none|colstrip,colstrip syn=none|colstrip maps=none caps=0"
    x = torch.randn(2, 36, 44, device="cuda")
    _, names = launched(P, lambda: p.wavedec(x))
    assert names == {"k_dwt2_ana"}, names
    _, names = launched(P, lambda: p.adjoint(torch.randn((2,) + p.rec_shape, device="cuda")))
    assert names == {"k_dwt2_ana"}, names
    # the neighbours on either side are the rows family's
    for near in (L - 2, L + 2):
        q = P.get_plan(2, (36, 44), 2, F.random_bank(near, near), "reflect", "cuda", flags=NO_PLANE)
        assert q.routes.startswith("ana=none|rows,rows adj=none|rows,rows"), (near, q.routes)


@pytest.mark.parametrize("wavelet", ["haar", "db3"])
def test_1d_synthesis_routes_at_8_and_9_levels(P, wavelet):
    """700 samples. J = 8 runs the persistent kernel, J = 9 the generic one, and both give the per-axis
    route's values. Bar: a level's output is a chain of L <= 6 FMAs, so a route rounds it by at most
    L * 2^-24 * sum |tap * input| <= 6 * 6e-8 * 2 * scale < 1e-6 * scale (the taps an output meets, half
    of rec_lo and half of rec_hi, have l1 norm < 2; scale = the largest coefficient or output). The
    half of rec_lo that carries a level's error to the next has l1 norm < 1 (haar 0.71, db3 0.98), so
    the error only adds up: two routes over J levels differ by at most 2 * J * 1e-6 * scale."""
    n, B = 700, 3
    for J, kernel in ((8, "k_dwt1_syn_int"), (9, "k_dwt1_syn")):
        p = P.get_plan(1, (n,), J, wavelet, "reflect", "cuda")
        axis = P.get_plan(1, (n,), J, wavelet, "reflect", "cuda", flags=GENERIC)
        assert p.routes.startswith("ana=tile1|") and " syn=tile1|" in p.routes, p.routes
        assert " syn=none|axis" in axis.routes, axis.routes
        torch.manual_seed(J)
        cf = axis.wavedec(torch.randn(B, n, device="cuda"))
        ref, names = launched(P, lambda: axis.waverec(cf, B, alphas=[0.5, 1.0]))
        assert names == {"k_synthesis_axis"}, names
        got, names = launched(P, lambda: p.waverec(cf, B, alphas=[0.5, 1.0]))
        assert names == {kernel}, (J, names)
        bar = 2 * J * 1e-6 * max(float(ref.abs().max()), float(cf.abs().max()))
        err = float((got - ref).abs().max())
        print("[dispatch] %s J=%d %s: |tile - axis| = %.3e, bar %.3e" % (wavelet, J, kernel, err, bar))
        assert float(ref.abs().max()) > 1.0                  # 3 x 700 normal samples come back: not a zero output
        assert err <= bar, (J, err, bar)


def test_an_odd_length_is_refused_at_plan_creation(P):
    from wam_amd import _lib, filters
    taps = (ctypes.c_double * 5)(0.1, 0.2, 0.3, 0.2, 0.1)
    shape = (ctypes.c_int64 * 1)(64)
    h = ctypes.c_void_p()
    P.timing_drain()
    P.timing_enable(True)
    rc = _lib.lib.wam_plan_create_ex(ctypes.byref(h), 1, shape, 1, taps, taps, taps, taps, 5,
                                     filters.mode_id("reflect"), 0)
    P.timing_enable(False)
    assert rc == UNSUPPORTED and not h.value and P.timing_drain() == []


def test_a_length_outside_every_list_launches_nothing(P):
    """22 taps: every transform of the plan is the per-axis kernels', and the fused ranked syntheses
    (the 1D tile and 2D plane families, forced with route 1) return WAM_ERR_UNSUPPORTED, leave the
    output alone and record no timer entry."""
    from wam_amd import _lib as L
    bank = F.random_bank(22, 22)
    p1 = P.get_plan(1, (300,), 2, bank, "reflect", "cuda")
    p2 = P.get_plan(2, (64, 64), 2, bank, "reflect", "cuda")
    p3 = P.get_plan(3, (24, 24, 24), 1, bank, "reflect", "cuda")
    assert p1.routes == "ana=none|axis,axis adj=none|axis,axis syn=none|axis maps=none caps=0"
    assert p2.routes == p1.routes
    assert p3.routes == "ana=none|axis adj=none|axis syn=none|axis maps=none caps=0"
    for p in (p1, p2, p3):
        cf, names = launched(P, lambda: p.wavedec(torch.randn((2,) + p.shape, device="cuda")))
        assert names == {"k_analysis_axis"}, names
        _, names = launched(P, lambda: p.waverec(cf, 2))
        assert names == {"k_synthesis_axis"}, names
    st = L.stream_of(torch.device("cuda"))
    n_iter, M = 4, 5
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    for p, sym, dims in ((p1, "wam_waverec1_ranked", (2,)), (p2, "wam_waverec2_ranked", (2, 1))):
        K, items = p.coeff_numel, int(np.prod(dims))
        assert getattr(L.lib, sym + "_route")(p.handle) == 0
        assert int(getattr(L.lib, sym + "_workspace_bytes")(p.handle, *dims, n_iter, 1)) <= ws.numel()
        cf = torch.randn(items * K, device="cuda")
        rank = torch.stack([torch.randperm(K) for _ in range(dims[0])]).to(torch.int32).cuda()
        pos = torch.arange(K, dtype=torch.int32, device="cuda")
        out = torch.full((items * M,) + p.rec_shape, 7.0, device="cuda")
        row_max = torch.full((items * M,), 7.0, device="cuda")
        extra = (L.ptr(row_max),) if sym == "wam_waverec1_ranked" else ()
        rc, names = launched(P, lambda: getattr(L.lib, sym)(p.handle, *dims, L.ptr(cf), L.ptr(rank), K, L.ptr(pos), n_iter,
                                                            K // n_iter, 0, 1, L.ptr(out), *extra, L.ptr(ws), st))
        assert rc == UNSUPPORTED and names == set(), (sym, rc, names)
        assert bool((out == 7.0).all()) and bool((row_max == 7.0).all())
