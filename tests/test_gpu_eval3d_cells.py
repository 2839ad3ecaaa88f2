"""wam_waverec_cells and wam_gaussian_filter3d at the C ABI.

wam_waverec_cells: the fused 3D Haar route (k_haar3_syn_cells) bit for bit against the expansion route,
the plan's own route and the two-step route the test builds itself (cells_ref below: a numpy float32
gather-multiply, then Plan.waverec); the expansion route alone against the float64 oracle where the fused
kernel does not apply. Outputs are prefilled with a sentinel and every voxel must have been written.
wam_gaussian_filter3d: bits against three 1-D reference passes (tests/evalkern_ref.gauss_pass, which
tests/test_eval3d_mu_ref.py pins to scipy.ndimage.gaussian_filter in bits), between guard words.

Bars: bits between the routes; the synthesis bar of tests/test_gpu_dwt.py, 4 * 2e-6 * max(1, |ref|max),
against oracle.dwt.waverec3. Measured on one MI355X (printed when the module finishes): route 0 against
the oracle at most 0.021 of its bar.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dwt
from tests import eval3d_ref as R
from tests import evalkern_ref as K

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, 1, 3
F32, F64 = np.float32, np.float64
WORST = {"dsyn": 0.0}
GUARD = 64


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()
    print("[eval3d cells] worst route 0 synthesis error / bar %.3f" % WORST["dsyn"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_case(shape, J, sets, n_masks, grid_len, wavelet="haar", seed=0, nan=False):
    """Random coefficients, a random slot map into [0, grid_len) with a few -1 and a few >= grid_len, and
    per set its own uniform masks in [-2, 2] with exact 0.0, 1.0 and -0.0 entries."""
    from wam_amd.plan import get_plan
    p = get_plan(3, shape, J, wavelet, "symmetric", "cuda")
    Kc = p.coeff_numel
    rng = np.random.RandomState(seed + 17 * J + n_masks + grid_len)
    coeffs = (rng.standard_normal(sets * Kc) * 3).astype(F32)
    slot = rng.randint(0, grid_len, Kc).astype(np.int32)
    odd = rng.choice(Kc, 9, replace=False)
    slot[odd[:4]] = -1
    slot[odd[4:7]] = grid_len
    slot[odd[7:]] = [grid_len + 1000, np.iinfo(np.int32).min]
    grid = rng.uniform(-2, 2, (sets, n_masks, grid_len)).astype(F32)
    pick = rng.uniform(size=grid.shape)
    grid[pick < 0.05] = F32(0.0)
    grid[(pick >= 0.05) & (pick < 0.10)] = F32(-0.0)
    grid[(pick >= 0.10) & (pick < 0.15)] = F32(1.0)
    assert (grid < 0).any() and (coeffs < 0).any() and (sets == 1 or not np.array_equal(grid[0], grid[-1]))
    if nan:                                   # a NaN coefficient of the last band of the last set meets a 0.0
        k = Kc - 3
        slot[k] = 5
        bn = p.band_offsets[-1] - p.band_offsets[-2]
        coeffs[sets * p.band_offsets[-2] + (sets - 1) * bn + (k - p.band_offsets[-2])] = np.nan
        grid[sets - 1, 0, 5] = F32(0.0)
    return p, Kc, coeffs, slot, grid


def cells_ref(band_off, sets, coeffs, slot, grid):
    """The masked sets of wam_waverec_cells' contract, flat band-major over sets * n_masks items, item
    (s, m) = s * n_masks + m: every value the single float32 product c * f, f = grid[s, m, slot] for a slot
    in [0, grid_len) and 1.0f otherwise."""
    n_masks, grid_len = grid.shape[1:]
    nb = len(band_off) - 1
    inr = (slot >= 0) & (slot < grid_len)
    f = np.where(inr[None, None, :], grid[:, :, np.where(inr, slot, 0)], F32(1.0)).astype(F32)   # [sets, n_masks, K]
    out = np.empty(sets * n_masks * band_off[nb], dtype=F32)
    with np.errstate(invalid="ignore"):
        for b in range(nb):
            bn = band_off[b + 1] - band_off[b]
            src = coeffs[sets * band_off[b]:sets * band_off[b + 1]].reshape(sets, 1, bn)
            o = sets * n_masks * band_off[b]
            out[o:o + sets * n_masks * bn] = (src * f[:, :, band_off[b]:band_off[b + 1]]).reshape(-1)
    assert out.dtype == F32
    return out


def cells(L, p, sets, dc, ds, dg, route, ws=True, out=None):
    """wam_waverec_cells through the C ABI -> (status, out); the output is prefilled with a sentinel."""
    n_masks, grid_len = dg.shape[1:]
    if out is None:
        out = torch.full((sets * n_masks,) + p.rec_shape, 7.0, device="cuda")
    nb = int(L.lib.wam_waverec_cells_workspace_bytes(p.handle, sets, n_masks, 0))
    w = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda") if ws else None
    rc = L.lib.wam_waverec_cells(p.handle, sets, L.ptr(dc), L.ptr(ds), n_masks, grid_len, L.ptr(dg), route, L.ptr(out),
                                 L.ptr(w), L.stream_of(out.device))
    torch.cuda.synchronize()
    return rc, out


def host(t):
    return t.cpu().numpy()


FUSED_CASES = {
    # fewer blocks than a wave; several sets in what would be one workgroup of a flat block index
    "8x8x8_J1": ((8, 8, 8), 1, 3, 4, 27, False),
    # 17 masks, different per set; a NaN coefficient
    "8x8x8_J2_m17": ((8, 8, 8), 2, 3, 17, 64, True),
    # non-cubic strides
    "8x12x16_J2": ((8, 12, 16), 2, 2, 5, 27, False),
    # several rows of blocks, five chunks
    "16x16x16_J2_m65": ((16, 16, 16), 2, 2, 65, 64, False),
    # enough work for the launcher to keep several masks per workgroup (the small cases above are cut down to
    # one): on 256 compute units chunks of 4 with a partial last one at J = 1, of 2 at J = 2
    "32x32x32_J1_m17": ((32, 32, 32), 1, 8, 17, 27, False),
    "32x32x32_J2_m33": ((32, 32, 32), 2, 16, 33, 64, False),
}


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_route_equals_expansion_route_in_bits(L, name):
    shape, J, sets, n_masks, grid_len, nan = FUSED_CASES[name]
    p, Kc, coeffs, slot, grid = make_case(shape, J, sets, n_masks, grid_len, nan=nan)
    dc, ds, dg = dev(coeffs), dev(slot), dev(grid)
    rc1, out1 = cells(L, p, sets, dc, ds, dg, 1, ws=False)         # route 1 reads no workspace
    rc0, out0 = cells(L, p, sets, dc, ds, dg, 0)
    assert rc0 == OK and rc1 == OK
    two_step = host(p.waverec(dev(cells_ref(list(p.band_offsets), sets, coeffs, slot, grid)), sets * n_masks)[0])
    assert np.isnan(two_step).any() == nan
    assert not bool((out0 == 7.0).any()) and not bool((out1 == 7.0).any())        # every voxel was written
    K.assert_bits(host(out0), two_step, name + " route 0 vs cells_ref + waverec", nan_as_value=True)
    K.assert_bits(host(out1), two_step, name + " route 1 vs cells_ref + waverec", nan_as_value=True)
    K.assert_bits(host(out1), host(out0), name + " route 1 vs route 0", nan_as_value=True)
    rc, own = cells(L, p, sets, dc, ds, dg, -1)
    assert rc == OK
    K.assert_bits(host(own), two_step, name + " own route", nan_as_value=True)


@pytest.mark.parametrize("name", ["8x8x8_J1", "8x12x16_J2"])
def test_all_ones_grid_is_the_plain_reconstruction(L, name):
    shape, J, sets, n_masks, grid_len, _ = FUSED_CASES[name]
    p, Kc, coeffs, slot, grid = make_case(shape, J, sets, n_masks, grid_len)
    dc, ds, dg = dev(coeffs), dev(slot), dev(np.ones_like(grid))
    plain = host(p.waverec(dc, sets)[0])
    for route in (0, 1):
        rc, out = cells(L, p, sets, dc, ds, dg, route)
        assert rc == OK
        got = host(out).reshape((sets, n_masks) + p.rec_shape)
        for m in range(n_masks):
            K.assert_bits(got[:, m], plain, "%s route %d mask %d of ones" % (name, route, m))


def test_python_wrapper_routes(L):
    """Plan.waverec_cells on the plan's own route and on both forced ones: the same bits."""
    p, Kc, coeffs, slot, grid = make_case((8, 8, 8), 2, 2, 5, 27)
    dc, ds, dg = dev(coeffs), dev(slot), dev(grid)
    outs = [p.waverec_cells(dc, 2, ds, dg, route=r) for r in (-1, 0, 1)]
    assert outs[0].shape == (10, 8, 8, 8)
    K.assert_bits(host(outs[0]), host(outs[1]), "wrapper own vs 0")
    K.assert_bits(host(outs[2]), host(outs[1]), "wrapper 1 vs 0")
    assert p.cells_route in (0, 1)
    with pytest.raises(ValueError):
        p.waverec_cells(dc, 2, ds, dg[:1])
    with pytest.raises(TypeError):
        p.waverec_cells(dc, 2, ds.long(), dg)


def test_grid_above_the_fused_limit_falls_back(L):
    """grid_len 65536, one above route 1's limit: route 1 declines with the sentinel intact, the own route runs route 0 in the workspace
    it was given and declines without one."""
    p, Kc, coeffs, slot, grid = make_case((8, 8, 8), 1, 1, 2, 65536)
    dc, ds, dg = dev(coeffs), dev(slot), dev(grid)
    rc, sentinel = cells(L, p, 1, dc, ds, dg, 1)
    assert rc == UNSUPPORTED and bool((sentinel == 7.0).all())
    rc0, out0 = cells(L, p, 1, dc, ds, dg, 0)
    rc, own = cells(L, p, 1, dc, ds, dg, -1)
    assert rc0 == OK and rc == OK
    K.assert_bits(host(own), host(out0), "fallback")
    if p.cells_route == 1:
        rc, sentinel = cells(L, p, 1, dc, ds, dg, -1, ws=False)
        assert rc == UNSUPPORTED and bool((sentinel == 7.0).all())
    K.assert_bits(host(p.waverec_cells(dc, 1, ds, dg)), host(out0), "wrapper fallback")


ROUTE0_CASES = {
    "haar_J3_16": ((16, 16, 16), 3, "haar"),
    "haar_J2_10": ((10, 10, 10), 2, "haar"),      # not divisible by 4
    "db2_J2_12": ((12, 12, 12), 2, "db2"),
}


@pytest.mark.parametrize("name", list(ROUTE0_CASES))
def test_expansion_route_against_the_oracle(L, name):
    shape, J, wavelet = ROUTE0_CASES[name]
    sets, n_masks, grid_len = 2, 3, 27
    p, Kc, coeffs, slot, grid = make_case(shape, J, sets, n_masks, grid_len, wavelet=wavelet, seed=5)
    assert p.cells_route == 0
    dc, ds, dg = dev(coeffs), dev(slot), dev(grid)
    rc, sentinel = cells(L, p, sets, dc, ds, dg, 1)
    assert rc == UNSUPPORTED and bool((sentinel == 7.0).all())
    rc, out = cells(L, p, sets, dc, ds, dg, 0)
    assert rc == OK
    rc, own = cells(L, p, sets, dc, ds, dg, -1)
    assert rc == OK
    K.assert_bits(host(own), host(out), name + " own route")
    off = list(p.band_offsets)
    masked = cells_ref(off, sets, coeffs, slot, grid).astype(F64)
    got = host(out)
    n = sets * n_masks
    assert got.shape == (n,) + p.rec_shape
    for i in range(n):
        bands = [masked[n * off[b] + i * (off[b + 1] - off[b]):n * off[b] + (i + 1) * (off[b + 1] - off[b])]
                 .reshape(p.band_shapes[b]) for b in range(p.nbands)]
        cont = [bands[0]] + [dict(zip(R.KEYS3, bands[1 + 7 * l:8 + 7 * l])) for l in range(J)]
        ref = dwt.waverec3(cont, wavelet)
        bar = 4 * 2e-6 * max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(got[i] - ref).max())
        WORST["dsyn"] = max(WORST["dsyn"], err / bar)
        assert err <= bar, (name, i, err, bar)


def test_argument_errors(L):
    from wam_amd.plan import get_plan
    p, Kc, coeffs, slot, grid = make_case((8, 8, 8), 1, 1, 4, 27)
    dc, ds, dg = dev(coeffs), dev(slot), dev(grid)
    out = torch.full((4, 8, 8, 8), 7.0, device="cuda")
    w = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    st = L.stream_of(out.device)

    def call(plan=p, sets=1, c=dc, s=ds, n_masks=4, grid_len=27, g=dg, route=-1, o=out, ws=w):
        return L.lib.wam_waverec_cells(plan.handle, sets, L.ptr(c), L.ptr(s), n_masks, grid_len, L.ptr(g), route, L.ptr(o),
                                       L.ptr(ws), st)
    p2 = get_plan(2, (16, 32), 1, "haar", "symmetric", "cuda")
    assert call(plan=p2) == UNSUPPORTED
    assert call(sets=-1) == INVALID
    assert call(n_masks=0) == INVALID
    assert call(grid_len=0) == INVALID
    for k in ("c", "s", "g", "o"):
        assert call(**{k: None}) == INVALID
    assert call(route=2) == INVALID and call(route=-2) == INVALID
    assert call(route=0, ws=None) == INVALID                                    # route 0 without a workspace
    assert call(route=0, ws=w[4:]) == INVALID                                   # ... or with a misaligned one
    assert call(n_masks=65536 * 16) == INVALID                                  # more chunks than the grid holds
    assert call(route=1, c=dc[1:]) == UNSUPPORTED                               # coeffs not 8-byte aligned
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                             # nothing was launched
    assert call(sets=0, ws=None) == OK                                          # no sets: nothing to do
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------ wam_gaussian_filter3d
class Guarded:
    """n float64 on the device between two guards of GUARD elements, all filled with the sentinel."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), K.SENTINEL, dtype=torch.float64, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == K.SENTINEL).all() and (self.buf[GUARD + self.n:] == K.SENTINEL).all())

    def untouched(self):
        return bool((self.buf == K.SENTINEL).all())


def gauss3(L, items, d, h, w, weights, radius, x, tmp, out):
    wc = np.ascontiguousarray(weights, dtype=F64)
    assert wc.size >= radius + 1
    rc = L.lib.wam_gaussian_filter3d(items, d, h, w, wc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), radius,
                                     L.ptr(x), L.ptr(tmp), L.ptr(out), L.stream_of(torch.device("cuda")))
    torch.cuda.synchronize()
    return rc


def gauss3_input(items, d, h, w):
    """items of different data: signed noise on a per-item ramp, a different scale per item."""
    rng = np.random.RandomState(100 * d + 10 * h + w)
    per_item = np.arange(items)[:, None, None, None]
    x = rng.standard_normal((items, d, h, w)) + np.linspace(-1, 2, d * h * w).reshape(1, d, h, w) * (1 + per_item)
    return np.ascontiguousarray(x * 1.5 ** per_item)


def gauss3_ref(x, wt, r):
    for axis in (1, 2, 3):
        x = K.gauss_pass(x, wt, r, axis)
    return x


# (items, d, h, w, sigma): non-cubic volumes, items of different data, extents below the radius (3 x 1 x 9 at
# sigma 2: radius 8 reflects several times), radius 32 on 4 x 6 x 5, more than one workgroup (16^3)
GAUSS3_CASES = [(3, 5, 7, 9, 2), (2, 8, 8, 8, 2), (1, 16, 12, 8, 2), (2, 3, 1, 9, 2), (1, 6, 10, 4, 1), (1, 4, 6, 5, 8),
                (2, 16, 16, 16, 2)]


@pytest.mark.parametrize("items,d,h,w,sigma", GAUSS3_CASES)
def test_gaussian_filter3d(L, items, d, h, w, sigma):
    x = gauss3_input(items, d, h, w)
    wt, r = K.gaussian_weights(sigma)
    xd = dev(x)
    keep = xd.clone()
    tmp, out = Guarded(x.size), Guarded(x.size)
    assert gauss3(L, items, d, h, w, wt, r, xd, tmp.t, out.t) == OK
    K.assert_bits(host(out.t).reshape(x.shape), gauss3_ref(x, wt, r), "gaussian3d %dx%dx%dx%d r=%d" % (items, d, h, w, r))
    assert out.guards_intact() and tmp.guards_intact() and torch.equal(xd.view(torch.int64), keep.view(torch.int64))


def test_gaussian_filter3d_wrapper_and_radius_0(L):
    from wam_amd.plan import gaussian_filter3d
    x = gauss3_input(2, 3, 7, 5)
    x[0, 0, 0, :4] = [0.0, -0.0, 5e-324, -2.5e-310]      # zeros of both signs and subnormals
    x[1, 2, 6, 4] = 1.7976931348623157e308
    xd = dev(x)
    tmp, out = Guarded(x.size), Guarded(x.size)
    assert gauss3(L, 2, 3, 7, 5, [1.0], 0, xd, tmp.t, out.t) == OK
    K.assert_bits(host(out.t).reshape(x.shape), x, "gaussian3d radius 0")
    assert out.guards_intact() and tmp.guards_intact()
    wt, r = K.gaussian_weights(2)
    x = gauss3_input(2, 5, 7, 9)
    K.assert_bits(host(gaussian_filter3d(dev(x), wt, r)), gauss3_ref(x, wt, r), "wrapper, items")
    K.assert_bits(host(gaussian_filter3d(dev(x[0]), wt, r)), gauss3_ref(x[:1], wt, r)[0], "wrapper, one volume")


def test_gaussian_filter3d_refusals_and_empty(L):
    x = gauss3_input(1, 4, 6, 5)
    xd = dev(x)
    tmp, out = Guarded(x.size), Guarded(x.size)
    w66 = np.full(66, 1.0 / 131)
    assert gauss3(L, 1, 4, 6, 5, w66, 65, xd, tmp.t, out.t) == INVALID
    assert gauss3(L, 1, 4, -6, 5, w66, 2, xd, tmp.t, out.t) == INVALID
    assert gauss3(L, 1, 4, 6, 5, w66, 2, xd, None, out.t) == INVALID
    assert gauss3(L, 1, 2048, 2048, 2048, w66, 2, xd, tmp.t, out.t) == INVALID     # more than INT32_MAX voxels
    assert gauss3(L, 0, 4, 6, 5, w66, 2, xd, tmp.t, out.t) == OK
    assert out.untouched() and tmp.untouched()
