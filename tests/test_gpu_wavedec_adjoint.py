"""The wavedec adjoint on the device (wam_wavedec_adjoint, Plan.wavedec_adjoint, autograd through
wam_amd.wavedec*) against autograd through the float64 CPU oracle.

Bar per case: max(4 * d32, 8e-6 * max(1, max|ref|)), d32 = how far the oracle's own float32 autograd lies
from its float64 run on the same inputs; the floor is the one test_gpu_dwt.py uses for waverec
(4 x 2e-6: one fp32 rounding per tap, two filter passes per axis pair)."""
import functools

import numpy as np
import pytest
import torch

from tests import wavedec_adjoint_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 8e-6


@pytest.fixture(scope="module")
def P():
    import wam_amd  # noqa: F401
    from wam_amd import plan
    assert torch.cuda.is_available()
    return plan


@functools.lru_cache(None)
def reference(case, mode, batch=2, seed=0):
    """(x, band grads, float64 oracle gradient, bar) of a case; computed once per session."""
    _, wavelet, _, levels = case
    x, grads = R.case_inputs(case, batch, seed)
    ref = R.oracle_gradient(x, grads, wavelet, mode, levels, torch.float64)
    d32 = np.abs(R.oracle_gradient(x, grads, wavelet, mode, levels, torch.float32) - ref).max()
    return x, grads, ref, max(4 * d32, FLOOR * max(1.0, np.abs(ref).max()))


def flat_of(grads):
    return torch.cat([torch.tensor(g, dtype=torch.float32).reshape(-1) for g in grads]).cuda()


def device_adjoint(P, case, mode, grads, generic):
    ndim, wavelet, shape, levels = case
    plan = P.get_plan(ndim, shape, levels, wavelet, mode, "cuda", generic=generic)
    batch = grads[0].shape[0]
    return plan, plan.wavedec_adjoint(flat_of(grads), batch).cpu().numpy().astype(np.float64)


def timed_names(P, fn):
    P.timing_drain()
    P.timing_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        P.timing_enable(False)
    return out, {r[0] for r in P.timing_drain()}


# ---------------------------------------------------------------- 1. the entry against the oracle
@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("mode", R.MODES)
def test_entry_matches_oracle_gradient(P, mode, generic):
    for case in R.CASES:
        x, grads, ref, bar = reference(case, mode)
        plan, got = device_adjoint(P, case, mode, grads, generic)
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        print("%s %s %s err=%.3g bar=%.3g" % (R.case_id(case), mode, plan.wavedec_adjoint_routes, err, bar))
        assert err <= bar, (R.case_id(case), mode, generic, err, bar)


# ---------------------------------------------------------------- 2. tile edges of the fold route
def edge_cases():
    out = []
    for wavelet, L in (("db4", 8), ("sym8", 16)):
        s = 130 - L  # output columns of one strip of the streaming synthesis
        p = L - 2
        out += [(2, wavelet, hw, 2) for hw in ((s - 1, s), (s, s + 1), (s + 1, s - 1))]
        out.append((2, wavelet, (p + 3, p + 4), 1))  # odd by even, p < n < 2p: the fold zones of both ends overlap
    return out


@pytest.mark.parametrize("mode", ["reflect", "symmetric", "periodic"])
@pytest.mark.parametrize("case", edge_cases(), ids=R.case_id)
def test_fold_route_tile_edges(P, case, mode):
    x, grads, ref, bar = reference(case, mode)
    fold_plan, fold = device_adjoint(P, case, mode, grads, False)
    axis_plan, axis = device_adjoint(P, case, mode, grads, True)
    assert set(fold_plan.wavedec_adjoint_routes) == {"fold2d"} and set(axis_plan.wavedec_adjoint_routes) == {"axis"}
    print("%s %s fold-axis=%.3g fold-ref=%.3g axis-ref=%.3g bar=%.3g" % (
        R.case_id(case), mode, np.abs(fold - axis).max(), np.abs(fold - ref).max(), np.abs(axis - ref).max(), bar))
    assert np.abs(fold - axis).max() <= 1e-5 * np.abs(axis).max()
    assert np.abs(fold - ref).max() <= bar
    assert np.abs(axis - ref).max() <= bar


# ---------------------------------------------------------------- 3. dot product with the device wavedec
@pytest.mark.parametrize("ndim,wavelet,shape,levels", [
    (2, "db4", (224, 224), 3), (2, "db4", (225, 223), 3), (2, "sym8", (96, 80), 3), (1, "db6", (4001,), 5),
    (3, "db2", (17, 18, 19), 2)], ids=lambda v: str(v).replace(" ", ""))
def test_dot_product(P, ndim, wavelet, shape, levels):
    plan = P.get_plan(ndim, shape, levels, wavelet, "reflect", "cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((2,) + shape, device="cuda", generator=g)
    c = torch.randn(2 * plan.coeff_numel, device="cuda", generator=g)
    lhs = float((plan.wavedec(x).double() * c.double()).sum())
    rhs = float((x.double() * plan.wavedec_adjoint(c, 2).double()).sum())
    print("lhs=%.9g rhs=%.9g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + np.sqrt(x.numel()))


# ---------------------------------------------------------------- 4. zero mode, orthogonal wavelets
@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("wavelet", ["haar", "db4", "sym8"])
def test_zero_mode_equals_cropped_waverec(P, wavelet, generic):
    for ndim, shape, levels in ((2, (20, 23), 2), (2, (9, 11), 2), (1, (37,), 3)):
        case = (ndim, wavelet, shape, levels)
        x, grads, ref, bar = reference(case, "zero")
        plan, got = device_adjoint(P, case, "zero", grads, generic)
        rec = plan.waverec(flat_of(grads), 2)[0]
        crop = rec[(slice(None),) + tuple(slice(0, n) for n in shape)].cpu().numpy().astype(np.float64)
        assert np.abs(got - crop).max() <= bar, (case, np.abs(got - crop).max(), bar)
        assert np.abs(got - ref).max() <= bar


# ---------------------------------------------------------------- 5. launch size
def test_launch_size_and_determinism(P):
    fold_plan = P.get_plan(2, (224, 224), 3, "db4", "reflect", "cuda")
    axis_plan = P.get_plan(2, (224, 224), 3, "db4", "reflect", "cuda", generic=True)
    assert fold_plan.wavedec_adjoint_routes == ["fold2d"] * 3 and axis_plan.wavedec_adjoint_routes == ["axis"] * 3
    c = torch.randn(192 * fold_plan.coeff_numel, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    fold, fold2 = fold_plan.wavedec_adjoint(c, 192), fold_plan.wavedec_adjoint(c, 192)
    axis, axis2 = axis_plan.wavedec_adjoint(c, 192), axis_plan.wavedec_adjoint(c, 192)
    assert fold.shape == (192, 224, 224)
    assert torch.equal(fold, fold2) and torch.equal(axis, axis2)
    assert float((fold - axis).abs().max()) <= 1e-5 * float(axis.abs().max())


# ---------------------------------------------------------------- 6. autograd
def _bands_of(coeffs, ndim):
    from wam_amd.constants import KEYS3
    if ndim == 1:
        return list(coeffs)
    if ndim == 2:
        return [coeffs[0]] + [t for lv in coeffs[1:] for t in lv]
    return [coeffs[0]] + [lv[k] for lv in coeffs[1:] for k in KEYS3]


@pytest.mark.parametrize("case", [(1, "db4", (37,), 3), (2, "sym8", (20, 23), 2), (3, "db2", (6, 7, 5), 1)],
                         ids=R.case_id)
def test_autograd_through_wavedec(P, case):
    import wam_amd
    ndim, wavelet, shape, levels = case
    x, grads, ref, bar = reference(case, "reflect")
    dec = {1: wam_amd.wavedec, 2: wam_amd.wavedec2, 3: wam_amd.wavedec3}[ndim]
    xt = torch.tensor(x, dtype=torch.float32, device="cuda", requires_grad=True)
    bands = _bands_of(dec(xt, wavelet, mode="reflect", level=levels), ndim)
    loss = sum((b * torch.tensor(g, dtype=torch.float32, device="cuda")).sum() for b, g in zip(bands, grads))
    (gx,) = torch.autograd.grad(loss, xt)
    assert np.abs(gx.cpu().numpy().astype(np.float64) - ref).max() <= bar


def test_unused_bands_give_zero_gradient(P):
    import wam_amd
    case = (2, "sym8", (20, 23), 2)
    x, grads, _, _ = reference(case, "reflect")
    used = [g if b in (0, 5) else np.zeros_like(g) for b, g in enumerate(grads)]
    ref = R.oracle_gradient(x, used, "sym8", "reflect", 2, torch.float64)
    d32 = np.abs(R.oracle_gradient(x, used, "sym8", "reflect", 2, torch.float32) - ref).max()
    xt = torch.tensor(x, dtype=torch.float32, device="cuda", requires_grad=True)
    bands = _bands_of(wam_amd.wavedec2(xt, "sym8", mode="reflect", level=2), 2)
    loss = sum((bands[b] * torch.tensor(grads[b], dtype=torch.float32, device="cuda")).sum() for b in (0, 5))
    (gx,) = torch.autograd.grad(loss, xt)
    assert np.abs(gx.cpu().numpy().astype(np.float64) - ref).max() <= max(4 * d32, FLOOR * max(1.0, np.abs(ref).max()))


def test_outputs_do_not_depend_on_requires_grad(P):
    import wam_amd
    x = torch.randn((2, 3, 33, 40), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    a = _bands_of(wam_amd.wavedec2(x, "db4", mode="reflect", level=2), 2)
    b = _bands_of(wam_amd.wavedec2(x.clone().requires_grad_(True), "db4", mode="reflect", level=2), 2)
    with torch.no_grad():
        c = _bands_of(wam_amd.wavedec2(x.clone().requires_grad_(True), "db4", mode="reflect", level=2), 2)
    assert all(not t.requires_grad for t in a + c) and all(t.requires_grad for t in b)
    assert all(torch.equal(u, v.detach()) and torch.equal(u, w) for u, v, w in zip(a, b, c))


def test_filtered_model_chain_matches_cpu_oracle(P):
    """x -> wavedec2 -> fixed mask -> waverec2 -> conv + tanh: d loss / d x against the same chain on the CPU
    oracle in float64."""
    import wam_amd
    from oracle import ptwt_torch as O
    rs = np.random.RandomState(11)
    x = rs.standard_normal((2, 3, 32, 32)).astype(np.float32)
    w = (0.2 * rs.standard_normal((4, 3, 3, 3))).astype(np.float32)
    r = rs.standard_normal((2, 4, 30, 30)).astype(np.float32)
    shapes = R.band_shapes((32, 32), 8, 2)
    masks = [(rs.uniform(size=(2, 3) + s) < 0.6).astype(np.float32) for s in shapes]

    def chain(mod, xt, dev, dtype):
        t = lambda a: torch.tensor(a, dtype=dtype, device=dev)
        co = mod.wavedec2(xt, "db4", mode="reflect", level=2)
        bands = [b * t(m) for b, m in zip(_bands_of(co, 2), masks)]
        y = mod.waverec2([bands[0], tuple(bands[1:4]), tuple(bands[4:7])], "db4")
        return (torch.tanh(torch.nn.functional.conv2d(y, t(w))) * t(r)).sum()

    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(chain(O, xr, "cpu", torch.float64), xr)
    xg = torch.tensor(x, device="cuda", requires_grad=True)
    (got,) = torch.autograd.grad(chain(wam_amd, xg, "cuda", torch.float32), xg)
    assert float((got.cpu().double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_create_graph_closes_both_pairs(P):
    import wam_amd
    gen = torch.Generator(device="cuda").manual_seed(4)
    rnd = lambda s: torch.randn(s, device="cuda", generator=gen)
    shapes = R.band_shapes((20, 23), 8, 2)
    # waverec: v = adjoint(g) as a function of g; d <v, c> / d g = waverec(c)
    leaves = [rnd((2,) + s).requires_grad_(True) for s in shapes]
    y = wam_amd.waverec2([leaves[0], tuple(leaves[1:4]), tuple(leaves[4:7])], "db4")
    g = rnd(tuple(y.shape)).requires_grad_(True)
    v = torch.autograd.grad(y, leaves, grad_outputs=g, create_graph=True)
    c = [rnd((2,) + s) for s in shapes]
    (gg,) = torch.autograd.grad(sum((a * b).sum() for a, b in zip(v, c)), g)
    want = wam_amd.waverec2([c[0], tuple(c[1:4]), tuple(c[4:7])], "db4")
    assert float((gg - want).abs().max()) <= 1e-6 * float(want.abs().max())
    # wavedec: v = wavedec_adjoint(g) as a function of g; d <v, c> / d g = wavedec(c)
    x = rnd((2, 20, 23)).requires_grad_(True)
    bands = _bands_of(wam_amd.wavedec2(x, "db4", mode="symmetric", level=2), 2)
    gs = [rnd(tuple(b.shape)).requires_grad_(True) for b in bands]
    (v,) = torch.autograd.grad(bands, x, grad_outputs=gs, create_graph=True)
    cx = rnd((2, 20, 23))
    ggs = torch.autograd.grad((v * cx).sum(), gs)
    want = _bands_of(wam_amd.wavedec2(cx, "db4", mode="symmetric", level=2), 2)
    for a, b in zip(ggs, want):
        assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------- 7. routes and the kernels that run
@pytest.mark.parametrize("ndim,wavelet,shape,levels,mode,generic,routes,names", [
    (2, "db4", (64, 72), 2, "reflect", False, ["fold2d", "fold2d"], {"k_dwt2_syn", "k_dwt2_adjoint_border"}),
    (2, "db4", (64, 72), 2, "zero", False, ["fold2d", "fold2d"], {"k_dwt2_syn"}),
    (2, "db4", (64, 72), 2, "reflect", True, ["axis", "axis"], {"k_analysis_adjoint_axis"}),
    (2, "db4", (6, 30), 1, "reflect", False, ["axis"], {"k_analysis_adjoint_axis"}),
    (1, "db6", (257,), 3, "reflect", False, ["axis"] * 3, {"k_analysis_adjoint_axis"}),
    (3, "db2", (17, 18, 19), 2, "reflect", False, ["axis"] * 2, {"k_analysis_adjoint_axis"}),
], ids=lambda v: str(v).replace(" ", "") if isinstance(v, tuple) else None)
def test_routes_announce_the_kernels(P, ndim, wavelet, shape, levels, mode, generic, routes, names):
    plan = P.get_plan(ndim, shape, levels, wavelet, mode, "cuda", generic=generic)
    assert plan.wavedec_adjoint_routes == routes
    c = torch.randn(2 * plan.coeff_numel, device="cuda")
    _, ran = timed_names(P, lambda: plan.wavedec_adjoint(c, 2))
    assert ran == names
