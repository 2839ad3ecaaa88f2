"""The numpy references of tests/epilogue_ref.py pinned to what already exists (numpy itself and the
float64 oracle), and the comparators of the GPU tests shown to reject seven mutants of a reference
-- the mistakes two HIP forms of one kernel could share -- on CPU data. No GPU."""
import numpy as np
import pytest

from tests import epilogue_ref as R

U = R.U
_trapz = getattr(np, "trapezoid", None) or np.trapz


# ------------------------------------------------------------------------------ shared data
class Data:
    """3 chained passes (groups 2, 3, 2) of 3 items over a 150-pixel frame with holes, 4 bands whose
    maxima differ by factors >= 1.5 per (group, band), distinct weights, an all-zero band with zero
    maximum in one group, a NaN and an inf map value, non-zero incoming accumulators."""
    n, F, K, nb = 3, 150, 170, 4
    passes = (2, 3, 2)

    def __init__(self):
        rng = np.random.RandomState(11)
        self.src, self.band, self.dst, self.cband = R.make_tables(rng, self.F, self.K, self.nb, 120)
        G = sum(self.passes)
        self.bmax = (0.5 * 1.5 ** np.arange(G * self.nb).reshape(G, self.nb)).astype(np.float32)
        u = rng.uniform(0.1, 1.0, (G * self.n, self.K)).astype(np.float32)
        self.maps = u * np.repeat(self.bmax, self.n, axis=0)[:, self.cband]
        # group 4, band 2: all zero with zero maximum
        self.maps[4 * self.n:5 * self.n, self.cband == 2] = 0.0
        self.bmax[4, 2] = 0.0
        valid = np.flatnonzero(self.src >= 0)
        ok = valid[self.band[valid] != 2]
        self.p_nan, self.p_inf = ok[3], ok[7]
        self.maps[1 * self.n + 1, self.src[self.p_nan]] = np.nan
        self.maps[5 * self.n + 2, self.src[self.p_inf]] = np.inf
        self.weights = rng.uniform(0.5, 1.5, G).astype(np.float32) * (1.0 + np.arange(G, dtype=np.float32))
        self.frame0 = rng.standard_normal((self.n, self.F))
        self.acc0 = rng.uniform(0.5, 1.0, (self.n, self.F)).astype(np.float32)
        self.prev0 = rng.uniform(0.5, 1.0, (self.n, self.F)).astype(np.float32)
        self.prev0[:, self.src < 0] = 0.0
        self.inf_mask = np.zeros((self.n, self.F), dtype=bool)
        self.inf_mask[2, self.p_inf] = True

    def steps(self, normalize=True, nan_to_num=True):
        """G[n, k, p] of the whole step sequence in float64, straight from the definition"""
        G = sum(self.passes)
        out = np.zeros((self.n, G, self.F))
        with np.errstate(divide="ignore", invalid="ignore"):
            for k in range(G):
                for p in np.flatnonzero(self.src >= 0):
                    v = self.maps[k * self.n:(k + 1) * self.n, self.src[p]].astype(np.float64)
                    out[:, k, p] = v / float(self.bmax[k, self.band[p]]) if normalize else v
        return np.nan_to_num(out, nan=0.0, posinf=R.FLT_MAX, neginf=-R.FLT_MAX) if nan_to_num else out

    def chain(self, fn, **kw):
        """run the 3 passes through fn(prev, acc, maps, bmax, groups, k0) -> (prev, acc)"""
        prev, acc, k0 = kw.pop("prev"), kw.pop("acc"), 0
        for g in self.passes:
            sl = slice(k0 * self.n, (k0 + g) * self.n)
            prev, acc = fn(prev, acc, self.maps[sl], self.bmax[k0:k0 + g], g, k0)
            k0 += g
        return prev, acc


@pytest.fixture(scope="module")
def d():
    return Data()


def _trapz_chain(d, dt, k0_of=lambda k0: k0, weights=False, fn=R.frame_trapz_ref):
    def one(prev, acc, maps, bmax, g, k0):
        w = d.weights[k0:k0 + g] if weights else None
        return fn(prev, acc, maps, bmax, d.src, d.band, g, k0_of(k0), d.n, True, weights=w, dt=dt)
    return d.chain(one, prev=np.zeros((d.n, d.F)), acc=np.zeros((d.n, d.F)))


# ------------------------------------------------------------------------------ pins
def test_tables_are_inverse(d):
    valid = d.src >= 0
    assert valid.sum() == 120 and (d.dst >= 0).sum() == 120
    assert np.array_equal(d.dst[d.src[valid]], np.flatnonzero(valid))
    assert np.array_equal(d.cband[d.src[valid]], d.band[valid])
    assert len(set(d.band[valid])) == d.nb


@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("size,levels", [(8, 1), (8, 3), (20, 3), (37, 2), (37, 4), (64, 5), (12, 3)])
def test_reproject_ref_vs_oracle(size, levels, approx):
    """half-pixel centres, edge clamp and the int(size / 2**j) splits against the float64 oracle
    (torch's bilinear interpolate): 1e-12 relative."""
    from oracle import wam_ref
    avg = np.random.RandomState(size + levels).standard_normal((2, size, size))
    ref = wam_ref.reproject_wam(avg, levels, approx)
    R.assert_within(R.reproject_ref(avg, levels, approx), ref, R.rel_bound(ref), "reproject_ref %d/%d" % (size, levels))


@pytest.mark.parametrize("size,levels", [(4, 3), (6, 3), (3, 2)])
def test_reproject_ref_raises_like_the_oracle(size, levels):
    from oracle import wam_ref
    with pytest.raises(RuntimeError):
        wam_ref.reproject_wam(np.ones((1, size, size)), levels, True)
    with pytest.raises(ValueError):
        R.reproject_ref(np.ones((1, size, size)), levels, True)


def test_frame_trapz_ref_vs_numpy_trapz(d):
    """3 chained passes carrying prev == np.trapz(np.nan_to_num(G), axis=1) of the whole sequence:
    float64 form to 1e-12, the fp32-emulated form within the trapezoid bound (inf pixel apart)."""
    G = d.steps()
    want = _trapz(G, axis=1)
    prev, acc = _trapz_chain(d, np.float64)
    R.assert_within(acc, want, R.rel_bound(want), "frame_trapz_ref f64 vs np.trapz")
    assert np.array_equal(prev, G[:, -1])
    K = G.shape[1]
    _, acc32 = _trapz_chain(d, np.float32)
    assert acc32.dtype == np.float32
    R.assert_within(acc32, want, (K + 2) * U * np.abs(G).sum(axis=1), "frame_trapz_ref f32 vs np.trapz",
                    exclude=d.inf_mask, max_excluded=0.01)


def test_frame_trapz_ref_weighted_and_accumulate_vs_sums(d):
    G = d.steps()
    _, acc = _trapz_chain(d, np.float64, weights=True)
    want = (G * d.weights.astype(np.float64)[None, :, None]).sum(axis=1)
    R.assert_within(acc, want, R.rel_bound(want), "frame_trapz_ref weighted")
    # SmoothGrad: NaN where a term is NaN (the NaN map value, the 0 / 0 band), holes untouched
    Gs = d.steps(nan_to_num=False)
    want = d.frame0 + Gs.sum(axis=1)
    k0, fr = 0, d.frame0
    for g in d.passes:
        fr = R.frame_accumulate_ref(fr, d.maps[k0 * d.n:(k0 + g) * d.n], d.bmax[k0:k0 + g], d.src, d.band, g, d.n, True)
        k0 += g
    R.assert_within(fr, want, R.rel_bound(want[np.isfinite(want)]), "frame_accumulate_ref", exclude=d.inf_mask)
    assert np.isnan(fr[:, (d.src >= 0) & (d.band == 2)]).all() and np.isnan(fr[1, d.p_nan])
    assert np.isnan(fr).sum() == d.n * ((d.src >= 0) & (d.band == 2)).sum() + 1
    assert np.array_equal(fr[:, d.src < 0], d.frame0[:, d.src < 0])


def test_cube_ref_mode2_vs_numpy_trapz_and_mode0_vs_loop(d):
    G = d.steps(normalize=False)
    want = _trapz(G, axis=1)
    one = lambda prev, acc, maps, bmax, g, k0: R.cube_ref(prev, acc, maps, d.src, g, k0, d.n, 2)
    prev, acc = d.chain(one, prev=d.prev0.astype(np.float64), acc=np.zeros((d.n, d.F)))
    R.assert_within(acc, want, R.rel_bound(want), "cube_ref mode 2 vs np.trapz")
    assert np.array_equal(prev, G[:, -1])
    # mode 0, fp32: the literal per-sample loop acc = (acc + v) / n_total on float32 scalars
    g = d.passes[0]
    _, got = R.cube_ref(None, d.acc0, d.maps[:g * d.n], d.src, g, 0, d.n, 0, n_total=7.0, dt=np.float32)
    want = d.acc0.copy()
    for n in range(d.n):
        for p in range(d.F):
            a = want[n, p]
            for s in range(g):
                v = d.maps[s * d.n + n, d.src[p]] if d.src[p] >= 0 else np.float32(0)
                a = np.float32(np.float32(a + v) / np.float32(7.0))
            want[n, p] = a
    R.assert_bits(got, want, "cube_ref mode 0 vs loop")


@pytest.mark.parametrize("C", [1, 3, 4])
def test_maps_ref_vs_numpy_mean(C):
    rng = np.random.RandomState(C)
    off = [0, 5, 12, 30]
    groups, gi = 3, 2
    items = groups * gi
    g = rng.standard_normal(items * C * off[-1]).astype(np.float32)
    maps, bmax = R.maps_ref(g, groups, gi, C, off, dt=np.float32)
    assert maps.dtype == np.float32 and bmax.dtype == np.float32
    for b in range(3):
        gb = g[items * C * off[b]:items * C * off[b + 1]].reshape(items, C, -1)
        want = np.abs(gb.mean(axis=1))
        assert want.dtype == np.float32
        R.assert_bits(maps[:, off[b]:off[b + 1]], want, "maps_ref band %d" % b)
        R.assert_bits(bmax[:, b], want.reshape(groups, -1).max(axis=1), "band_max %d" % b)
    m64, _ = R.maps_ref(g, groups, gi, C, off)
    R.assert_within(maps, m64, (C + 1) * U * R.maps_abs_sum(g, items, C, off) / C, "maps_ref f32 vs f64")


def test_stream_refs_vs_numpy():
    rng = np.random.RandomState(5)
    src = rng.standard_normal((7, 33)).astype(np.float32)
    acc = rng.standard_normal(33).astype(np.float32)
    got = R.accumulate_ref(acc, src, 7, 25.0)
    R.assert_within(got, (acc.astype(np.float64) + src.astype(np.float64).sum(axis=0)) / 25.0, 1e-14, "accumulate_ref")
    p, a = R.trapz_stream_ref(np.zeros(33), np.zeros(33), src[:3], 3, 0)
    p, a = R.trapz_stream_ref(p, a, src[3:], 4, 3)
    R.assert_within(a, _trapz(src.astype(np.float64), axis=0), 1e-14, "trapz_stream_ref")
    x = rng.standard_normal(40).astype(np.float32)
    assert np.array_equal(R.sigma_ref(x, 4, 10, 7, 0.15), np.float32(0.15) * np.ptp(x.reshape(4, 10)[:, :7], axis=1))


# ------------------------------------------------------------------------------ mutants
def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_comparator_rejects_wrong_band_max(d):
    """band maximum taken from group s+-1; band index of a neighbouring pixel"""
    g = 4  # the groups before the all-zero band: the mutants are rejected by value, not by a NaN
    maps, bmax = d.maps[:g * d.n], d.bmax[:g]
    ref = R.frame_accumulate_ref(d.frame0, maps, bmax, d.src, d.band, g, d.n, True)
    vmax = np.zeros((d.n, d.F))
    for s in range(g):
        valid, v = R._mosaic_values(maps, bmax, d.src, d.band, s, d.n, True, np.float64)
        vmax[:, valid] = np.fmax(vmax[:, valid], np.abs(v))
    bound = 2 * g * U * vmax + 1e-15 * np.abs(ref)
    emu = R.frame_accumulate_ref(d.frame0, maps, bmax, d.src, d.band, g, d.n, True, emulate=True)
    R.assert_within(emu, ref, bound, "emulated accumulate vs f64")
    for shift in (1, -1):
        mut = R.frame_accumulate_ref(d.frame0, maps, np.roll(bmax, shift, axis=0), d.src, d.band, g, d.n, True)
        _rejects(lambda: R.assert_within(mut, ref, bound, "mutant: band max of group s%+d" % shift))
    mut = R.frame_accumulate_ref(d.frame0, maps, bmax, d.src, np.roll(d.band, 1), g, d.n, True)
    _rejects(lambda: R.assert_within(mut, ref, bound, "mutant: neighbour's band"))
    # the trapezoid form of the same two
    G = d.steps()
    tb = (G.shape[1] + 2) * U * np.abs(G).sum(axis=1)
    _, tref = _trapz_chain(d, np.float64)

    def rolled(prev, acc, maps, bmax, src, band, g, k0, n, norm, weights=None, dt=np.float64):
        return R.frame_trapz_ref(prev, acc, maps, bmax, src, np.roll(band, 1), g, k0, n, norm, weights=weights, dt=dt)
    _, mut = _trapz_chain(d, np.float64, fn=rolled)
    _rejects(lambda: R.assert_within(mut, tref, tb, "mutant: neighbour's band (trapz)", exclude=d.inf_mask))


def test_comparator_rejects_k0_dropped(d):
    """`k0 + s > 0` replaced by `s > 0`: the first step of every later pass loses its trapezoid"""
    G = d.steps()
    bound = (G.shape[1] + 2) * U * np.abs(G).sum(axis=1)
    _, ref = _trapz_chain(d, np.float64)
    _, emu = _trapz_chain(d, np.float32)
    R.assert_within(emu, ref, bound, "emulated trapz vs f64", exclude=d.inf_mask)
    _, mut = _trapz_chain(d, np.float64, k0_of=lambda k0: 0)
    _rejects(lambda: R.assert_within(mut, ref, bound, "mutant: s > 0", exclude=d.inf_mask))
    _, mut32 = _trapz_chain(d, np.float32, k0_of=lambda k0: 0)
    _rejects(lambda: R.assert_bits(mut32, emu, "mutant: s > 0 (bits)"))


def test_comparator_rejects_nan_to_num_before_division(d):
    def early(prev, acc, maps, bmax, src, band, g, k0, n, norm, weights=None, dt=np.float64):
        return R.frame_trapz_ref(prev, acc, np.nan_to_num(maps, nan=0.0, posinf=R.FLT_MAX), bmax, src, band, g, k0, n,
                                 norm, weights=weights, dt=dt)

    def no_late(v):
        return v
    G = d.steps()
    bound = (G.shape[1] + 2) * U * np.abs(G).sum(axis=1)
    _, ref = _trapz_chain(d, np.float64)
    _, emu = _trapz_chain(d, np.float32)
    keep, R._nan_to_num = R._nan_to_num, no_late
    try:
        _, mut = _trapz_chain(d, np.float64, fn=early)
        _, mut32 = _trapz_chain(d, np.float32, fn=early)
    finally:
        R._nan_to_num = keep
    # the 0 / 0 band stays NaN, and the inf pixel becomes FLT_MAX / max instead of FLT_MAX
    _rejects(lambda: R.assert_within(mut, ref, bound, "mutant: nan_to_num first", exclude=d.inf_mask))
    _rejects(lambda: R.assert_bits(mut32, emu, "mutant: nan_to_num first (inf pixel)", only=d.inf_mask))


def test_comparator_rejects_mode0_divided_once(d):
    g, nt = d.passes[1], 7.0
    maps = d.maps[:g * d.n]
    _, ref = R.cube_ref(None, d.acc0, maps, d.src, g, 0, d.n, 0, n_total=nt)
    vmax = np.zeros((d.n, d.F))
    vmax[:, d.src >= 0] = np.abs(maps.reshape(g, d.n, -1)[:, :, d.src[d.src >= 0]]).max(axis=0)
    bound = 4 * U * np.maximum(np.abs(d.acc0), vmax)
    _, emu = R.cube_ref(None, d.acc0, maps, d.src, g, 0, d.n, 0, n_total=nt, dt=np.float32)
    R.assert_within(emu, ref, bound, "emulated mode 0 vs f64")
    _, summed = R.cube_ref(None, d.acc0, maps, d.src, g, 0, d.n, 0, n_total=1.0)
    _rejects(lambda: R.assert_within(summed / nt, ref, bound, "mutant: mode 0 divided once"))


def test_comparator_rejects_scale_on_sum_only():
    rng = np.random.RandomState(9)
    src = rng.standard_normal((7, 257)).astype(np.float32)
    acc = rng.uniform(0.5, 1.0, 257).astype(np.float32)
    ref = R.accumulate_ref(acc, src, 7, 25.0)
    bound = 8 * U * (np.abs(acc) + np.abs(src).sum(axis=0)) / 25.0
    R.assert_within(R.accumulate_ref(acc, src, 7, 25.0, dt=np.float32), ref, bound, "emulated accumulate_f32 vs f64")
    mut = acc.astype(np.float64) + R.accumulate_ref(np.zeros(257), src, 7, 25.0)
    _rejects(lambda: R.assert_within(mut, ref, bound, "mutant: scale on the sum only"))


def test_comparator_rejects_approx_on_item0():
    """disentangle_scales writes the approximation for the LAST item only (the oracle's stale loop
    index); written for item 0 instead it must fail the 1e-5 bar of the GPU test."""
    from oracle import wam_ref
    rng = np.random.RandomState(3)
    grads = [rng.standard_normal((3, 3, 5, 5)).astype(np.float32)] + [
        tuple(rng.standard_normal((3, 3, m, m)).astype(np.float32) for _ in range(3)) for m in (5, 10)]
    ref = wam_ref.disentangle_scales_2d(grads, 2, True)
    assert np.abs(ref[2, 2]).max() > 0.1 and not ref[:2, 2].any()
    mut = ref.copy()
    mut[0, 2], mut[2, 2] = ref[2, 2], 0.0
    R.assert_within(ref.copy(), ref, 1e-5, "disentangle identity")
    _rejects(lambda: R.assert_within(mut, ref, 1e-5, "mutant: approximation on item 0"))
