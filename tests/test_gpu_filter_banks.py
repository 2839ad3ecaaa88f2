"""Every DWT kernel route on filter banks whose stored sets differ (tests/filter_banks.py): random banks with
four unrelated filters and the table's biorthogonal wavelets, against the float64 references that
tests/test_filter_banks_ref.py pins to PyWavelets. With an orthogonal wavelet the plan's ANA, SYN and ADJ sets
hold the same numbers and hi is the mirror of lo, so a launcher reading the wrong set or a kernel indexing its
taps mirrored passes every other GPU test; here each such mistake lies more than 1000 bars from the reference.

Bars (the project's own): analysis 2e-6 * max(1, max|ref|) per band (test_gpu_dwt.py), waverec and its adjoint
4 x that, the wavedec adjoint 8e-6 * max(1, max|ref|) (test_gpu_wavedec_adjoint.py), maps 2e-6 * max(band_max).
Every test prints its worst error / bar.
"""
import functools
import re
import zlib

import numpy as np
import pytest
import torch

from tests import filter_banks as F

pytestmark = pytest.mark.gpu

TOL = 2e-6
B = 3
ALPHAS = [0.25, 1.0]
DENSE_MAX = 1100     # longest axis whose dense wavedec-adjoint reference is built
CAP_NOISY, CAP_MAPS, CAP_BF16 = 1, 2, 4
WORST = {}


def _caps(c):
    return int(re.search(r"caps=(\d+)", c.routes).group(1))


def _with(cap):
    return [c for c in F.CASES if _caps(c) & cap]


@pytest.fixture(scope="module")
def P():
    import wam_amd  # noqa: F401
    from wam_amd import plan
    assert torch.cuda.is_available()
    yield plan
    print("[filter-banks] worst error / bar per check: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def plan_of(P, c):
    p = P.get_plan(c.ndim, c.shape, c.J, F.get_bank(c.bank), c.mode, "cuda", flags=c.flags)
    # test_gpu_routes.py ties these strings to the kernels that launch
    assert p.routes == c.routes and p.wavedec_adjoint_routes == list(c.wa)
    return p


@functools.lru_cache(None)
def inputs(c):
    """(x, coefficient bands, gradient) of a case: float32-representable standard normals as float64"""
    L = F.bank_length(c)
    rs = np.random.RandomState(zlib.crc32(F.case_id(c).encode()) & 0x7FFFFFFF)
    x = F.f32(rs.standard_normal((B,) + c.shape))
    bands = [F.f32(rs.standard_normal((B,) + s)) for s in F.band_shapes(c.shape, L, c.J)]
    g = F.f32(rs.standard_normal((B,) + F.rec_shape(c.shape, L, c.J)))
    return x, bands, g


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def flat_dev(bands):
    return dev(F.flat_of(bands))


def host_bands(p, flat, batch):
    return [b.cpu().numpy().astype(np.float64) for b in p.split(flat, batch)]


def check(c, what, got, ref, bar):
    """max |got - ref| <= bar * max(1, max|ref|); records and prints error / bar"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (F.case_id(c), what, got.shape, ref.shape)
    ratio = float(np.abs(got - ref).max() / (bar * max(1.0, float(np.abs(ref).max()))))
    key = what.split()[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("[filter-banks] %s %s: error / bar = %.3g" % (F.case_id(c), what, ratio))
    assert ratio <= 1.0, (F.case_id(c), what, ratio)


def launched(P, fn):
    P.timing_drain()
    P.timing_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        P.timing_enable(False)
    return out, {r[0] for r in P.timing_drain()}


# ------------------------------------------------------------------------------ 1. wavedec
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_wavedec(P, case):
    p = plan_of(P, case)
    x, _, _ = inputs(case)
    if case.shape == (33000,):  # the interior-tile kernel, not only the boundary tiles' one
        flat, names = launched(P, lambda: p.wavedec(dev(x)))
        assert any(n.startswith("k_dwt1_ana_int") for n in names), names
    else:
        flat = p.wavedec(dev(x))
    got = host_bands(p, flat, B)
    ref = F.ref_wavedec(x, F.get_bank(case.bank), case.J, case.mode)
    assert len(got) == len(ref) == p.nbands
    for b, (g, r) in enumerate(zip(got, ref)):
        check(case, "wavedec band %d" % b, g, r, TOL)


# ------------------------------------------------------------------------------ 2. waverec
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_waverec_of_random_coefficients(P, case):
    p = plan_of(P, case)
    _, bands, _ = inputs(case)
    ref = F.ref_waverec(bands, F.get_bank(case.bank), case.ndim)
    flat = flat_dev(bands)
    out = p.waverec(flat, B)
    assert out.shape == (1, B) + p.rec_shape
    check(case, "waverec", out[0].cpu().numpy(), ref, 4 * TOL)
    out = p.waverec(flat, B, alphas=ALPHAS)
    assert out.shape == (len(ALPHAS), B) + p.rec_shape
    for i, a in enumerate(ALPHAS):  # the alphas are exact in fp32 and the synthesis is linear
        check(case, "waverec alpha %g" % a, out[i].cpu().numpy(), float(np.float32(a)) * ref, 4 * TOL)


# ------------------------------------------------------------------------------ 3. waverec's adjoint
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_adjoint(P, case):
    p = plan_of(P, case)
    _, _, g = inputs(case)
    got = host_bands(p, p.adjoint(dev(g)), B)
    ref = F.ref_adjoint(g, F.get_bank(case.bank), case.J)
    assert len(got) == len(ref)
    for b, (gb, rb) in enumerate(zip(got, ref)):
        check(case, "adjoint band %d" % b, gb, rb, 4 * TOL)


# ------------------------------------------------------------------------------ 4. wavedec's adjoint
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_wavedec_adjoint(P, case):
    p = plan_of(P, case)
    x, bands, _ = inputs(case)
    w = F.get_bank(case.bank)
    got = p.wavedec_adjoint(flat_dev(bands), B).cpu().numpy().astype(np.float64)
    assert got.shape == x.shape
    if max(case.shape) <= DENSE_MAX:
        check(case, "wavedec_adjoint", got, F.ref_wavedec_adjoint(bands, case.shape, w, case.J, case.mode), 4 * TOL)
        return
    # the dense reference is too large: <wavedec(x), c> == <x, wavedec_adjoint(c)>, the bar of test_dot_product
    lhs = sum(float((r * c).sum()) for r, c in zip(F.ref_wavedec(x, w, case.J, case.mode), bands))
    rhs = float((x * got).sum())
    ratio = abs(lhs - rhs) / (1e-5 * (abs(lhs) + np.sqrt(x.size)))
    print("[filter-banks] %s wavedec_adjoint dot: lhs=%.9g rhs=%.9g error / bar = %.3g" % (F.case_id(case), lhs, rhs,
                                                                                          ratio))
    WORST["wavedec_adjoint_dot"] = max(WORST.get("wavedec_adjoint_dot", 0.0), ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------ 5. the fused maps pass
@pytest.mark.parametrize("case", _with(CAP_MAPS), ids=F.case_id)
def test_adjoint_maps(P, case):
    p = plan_of(P, case)
    assert p.caps & P.CAP_ADJOINT_MAPS
    G, N, C = 2, 2, 3
    rs = np.random.RandomState(zlib.crc32(F.case_id(case).encode()) % 1000 + 1)
    g = F.f32(rs.standard_normal((G * N * C,) + p.rec_shape))
    gd = dev(g)
    maps, bmax, full = p.adjoint_maps(gd, G, N, C, full=True)
    assert torch.equal(full, p.adjoint(gd))
    rmaps, rbmax = F.ref_maps(F.ref_adjoint(g, F.get_bank(case.bank), case.J), G, N, C, p.band_offsets)
    scale = float(rbmax.max())
    for what, got, ref in (("maps", maps.view(G * N, -1), rmaps), ("maps band_max", bmax, rbmax)):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape
        ratio = float(np.abs(got - ref).max() / (TOL * scale))
        WORST["maps"] = max(WORST.get("maps", 0.0), ratio)
        print("[filter-banks] %s %s: error / bar = %.3g" % (F.case_id(case), what, ratio))
        assert ratio <= 1.0, (F.case_id(case), what, ratio)


# ------------------------------------------------------------------------------ 6. the noisy analysis
@pytest.mark.parametrize("case", _with(CAP_NOISY), ids=F.case_id)
def test_noisy_wavedec_reads_the_same_taps(P, case):
    """wavedec_noisy == wavedec(noise_add(x)) bit for bit: the noisy instantiations read the analysis set"""
    p = plan_of(P, case)
    assert p.caps & P.CAP_NOISY_WAVEDEC
    S, N, C = 2, 2, (3 if case.ndim == 2 else 1)
    n = int(np.prod(case.shape))
    torch.manual_seed(17)
    x = torch.randn((N, C) + case.shape, device="cuda")
    sigma = P.item_sigma(x, C * n, C * n, 0.25)
    fused = p.wavedec_noisy(x, sigma, S, N, C, seed=4321, sample_base=3)
    noisy = P.noise_add(x, sigma, S, N, C * n, C * n, seed=4321, sample_base=3)
    assert not torch.equal(noisy.view((S, N, C) + case.shape)[0], x)
    assert torch.equal(fused, p.wavedec(noisy.view((S * N * C,) + case.shape)))


# ------------------------------------------------------------------------------ 7. the bf16 hand-off
@pytest.mark.parametrize("case", _with(CAP_BF16), ids=F.case_id)
def test_bf16_handoff(P, case):
    """as tests/test_gpu_handoff.py states them: the bf16 NHWC synthesis is the fp32 one cast, and the bf16 maps
    entry equals the fp32 one on bf16-representable gradients"""
    p = plan_of(P, case)
    assert p.caps & P.CAP_BF16_NHWC
    N, C = 3, 3
    torch.manual_seed(31)
    cf = torch.randn(N * C * p.coeff_numel, device="cuda") * 3.0
    for al in (None, [0.0, 0.3, 1.0]):
        k = 1 if al is None else len(al)
        ref = p.waverec(cf, N * C, alphas=al).view((k * N, C) + p.rec_shape)
        got = p.waverec_bf16_nhwc(cf, N * C, C, alphas=al)
        assert got.dtype == torch.bfloat16 and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, ref.to(torch.bfloat16).contiguous(memory_format=torch.channels_last))
    g = (torch.randn((N, C) + p.rec_shape, device="cuda") * 1e-3).to(torch.bfloat16)
    g = g.contiguous(memory_format=torch.channels_last)
    maps, bmax, _ = p.adjoint_maps(g, 1, N, C)
    rmaps, rbmax, _ = p.adjoint_maps(g.float().contiguous().view((N * C,) + p.rec_shape), 1, N, C)
    assert torch.equal(maps, rmaps) and torch.equal(bmax, rbmax)


# ------------------------------------------------------------------------------ the ptwt-shaped layer
def test_autograd_with_a_wavelet_object(P):
    """wam_amd.wavedec2 / waverec2 called with a filters.Wavelet: the leaf gradients are the references of
    checks 3 and 4, so the object reaches the plan intact, and the plan cache is keyed on the taps: a second
    object of the same name with other taps gives its own answer."""
    import wam_amd
    w = F.random_bank(8, 8)
    shape, J, mode = (20, 23), 2, "reflect"
    rs = np.random.RandomState(88)
    case = F.Case(2, shape, J, 8, mode, 0, "", ())
    x = F.f32(rs.standard_normal((2, 3) + shape))
    shapes = F.band_shapes(shape, 8, J)
    gb = [F.f32(rs.standard_normal((2, 3) + s)) for s in shapes]
    xt = dev(x).requires_grad_(True)
    co = wam_amd.wavedec2(xt, w, mode=mode, level=J)
    bands = [co[0]] + [t for lv in co[1:] for t in lv]
    ref = F.ref_wavedec(x.reshape((6,) + shape), w, J, mode)
    for b, (t, r) in enumerate(zip(bands, ref)):
        check(case, "wavedec band %d (wavedec2)" % b, t.detach().cpu().numpy().reshape(r.shape), r, TOL)
    (gx,) = torch.autograd.grad(sum((t * dev(g)).sum() for t, g in zip(bands, gb)), xt)
    want = F.ref_wavedec_adjoint([g.reshape((6,) + s) for g, s in zip(gb, shapes)], shape, w, J, mode)
    check(case, "wavedec_adjoint (autograd)", gx.cpu().numpy().reshape(want.shape), want, 4 * TOL)
    # waverec2 of leaves: the gradient of <waverec2(c), g> with respect to c is the adjoint of g
    leaves = [dev(g).requires_grad_(True) for g in gb]
    rec = wam_amd.waverec2([leaves[0], tuple(leaves[1:4]), tuple(leaves[4:7])], w)
    rref = F.ref_waverec([g.reshape((6,) + s) for g, s in zip(gb, shapes)], w, 2)
    check(case, "waverec (waverec2)", rec.detach().cpu().numpy().reshape(rref.shape), rref, 4 * TOL)
    go = F.f32(rs.standard_normal(rref.shape))
    grads = torch.autograd.grad((rec * dev(go).view(rec.shape)).sum(), leaves)
    for b, (t, r) in enumerate(zip(grads, F.ref_adjoint(go, w, J))):
        check(case, "adjoint band %d (autograd)" % b, t.cpu().numpy().reshape(r.shape), r, 4 * TOL)
    # same name, other taps: must not be served by the first object's plan
    other = F.random_bank(8, 9)._replace(name=w.name)
    assert other != w
    co2 = wam_amd.wavedec2(dev(x), other, mode=mode, level=J)
    check(case, "wavedec band 0 (other taps)", co2[0].cpu().numpy().reshape(ref[0].shape),
          F.ref_wavedec(x.reshape((6,) + shape), other, J, mode)[0], TOL)
