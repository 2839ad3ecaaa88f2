"""The kernels a plan launches are the ones its route table names (Plan.routes / wam_plan_describe):
wavedec, the adjoint, waverec with IG alphas and the fused maps pass run with live timing on, and the
set of kernel names that ran must be exactly what the routes map to. Small shapes, one per kernel
family and per narrowing plan flag; a call the whole-transform kernel declines (an input that is not
16-byte aligned) must run on the per-level route and give the same bits."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ANA = {"plane": "k_plane_ana", "rows": "k_ana_rows", "colstrip": "k_dwt2_ana", "tile1": "k_dwt1_ana",
       "haar3": "k_haar3_ana", "tile3": "k_dwt3_ana_tile", "axis": "k_analysis_axis"}
SYN = {"plane": "k_plane_syn", "colstrip": "k_dwt2_syn", "tile1": "k_dwt1_syn", "haar3": "k_haar3_syn",
       "tile3": "k_dwt3_syn_tile", "axis": "k_synthesis_axis"}
MAPS = {"plane": "k_plane_maps", "rows": "k_adj_maps"}

# (ndim, shape, levels, wavelet, mode, flags)
PLANS = [
    (2, (32, 32), 2, "db4", "reflect", 0),
    (2, (30, 26), 2, "db3", "zero", 0),        # width not a multiple of 4
    (2, (24, 40), 2, "db5", "reflect", 0),     # 10 taps: column strips only
    (1, (1000,), 3, "db6", "reflect", 0),
    (3, (16, 16, 16), 2, "haar", "symmetric", 0),
    (3, (9, 10, 11), 1, "db2", "symmetric", 0),
    (2, (32, 32), 2, "db4", "reflect", 1),     # WAM_PLAN_GENERIC
    (2, (32, 32), 2, "db4", "reflect", 2),     # WAM_PLAN_NO_ROWS
    (2, (32, 32), 2, "db4", "reflect", 4),     # WAM_PLAN_NO_PLANE
]


@pytest.fixture(scope="module")
def wam():
    from wam_amd import plan
    assert torch.cuda.is_available()
    return plan


def _routes(p):
    m = re.fullmatch(r"ana=(\w+)\|([\w,]+) adj=(\w+)\|([\w,]+) syn=(\w+)\|(\w+) maps=(\w+) caps=(\d+)", p.routes)
    assert m, p.routes
    ana_w, ana_l, adj_w, adj_l, syn_w, syn_l, maps, caps = m.groups()
    assert int(caps) == p.caps
    return {"ana": (ana_w, ana_l.split(",")), "adj": (adj_w, adj_l.split(",")), "syn": (syn_w, [syn_l]), "maps": maps}


def _launched(P, fn):
    """fn's result and the names of the kernels it launched: template tags dropped, the 1D tile
    kernels' interior / boundary / persistent forms folded to their family name"""
    P.timing_drain()
    P.timing_enable(True)
    out = fn()
    torch.cuda.synchronize()
    P.timing_enable(False)
    names = {re.sub(r"^(k_dwt1_(ana|syn)).*", r"\1", r[0].split("<")[0]) for r in P.timing_drain()}
    return out, names


def _expected(route, table, levels_only=False):
    whole, levels = route
    if whole != "none" and not levels_only:
        return {table[whole]}
    return {table[lv] for lv in levels}


@pytest.mark.parametrize("ndim,shape,J,wav,mode,flags", PLANS)
def test_launched_kernels_are_the_routes(wam, ndim, shape, J, wav, mode, flags):
    P = wam
    p = P.get_plan(ndim, shape, J, wav, mode, "cuda", flags=flags)
    r = _routes(p)
    assert len(r["ana"][1]) == J and len(r["adj"][1]) == J
    torch.manual_seed(70)
    B = 3
    x = torch.randn((B,) + tuple(shape), device="cuda")
    cf, names = _launched(P, lambda: p.wavedec(x))
    assert names == _expected(r["ana"], ANA), (p.routes, names)
    g = torch.randn((B,) + p.rec_shape, device="cuda")
    _, names = _launched(P, lambda: p.adjoint(g))
    assert names == _expected(r["adj"], ANA), (p.routes, names)
    _, names = _launched(P, lambda: p.waverec(cf, B, alphas=[0.25, 1.0]))
    assert names == _expected(r["syn"], SYN), (p.routes, names)
    assert (r["maps"] != "none") == bool(p.caps & P.CAP_ADJOINT_MAPS)
    if r["maps"] != "none":
        _, names = _launched(P, lambda: p.adjoint_maps(g, 1, 1, 3))
        assert names == {MAPS[r["maps"]]}, (p.routes, names)


def test_declined_call_runs_the_level_routes(wam):
    """An input one float past a 16-byte boundary: the plane kernel declines the call, the per-level
    route's kernels run instead, and the coefficients equal the aligned call's bit for bit."""
    P = wam
    p = P.get_plan(2, (32, 32), 2, "db4", "reflect", "cuda")
    r = _routes(p)
    assert r["ana"][0] == "plane", p.routes
    torch.manual_seed(71)
    B = 3
    buf = torch.randn(B * 32 * 32 + 1, device="cuda")
    off = buf[1:].view(B, 32, 32)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    aligned = off.clone()
    assert aligned.data_ptr() % 16 == 0
    ref, names = _launched(P, lambda: p.wavedec(aligned))
    assert names == {"k_plane_ana"}, names
    got, names = _launched(P, lambda: p.wavedec(off))
    assert names == _expected(r["ana"], ANA, levels_only=True), (p.routes, names)
    assert torch.equal(got, ref)
