"""The epilogue kernels (wam_amd/csrc/epilogue.hip) against the plain-numpy references of
tests/epilogue_ref.py at the C ABI, one entry at a time, on synthetic injective mosaic tables.

Two assertions (u = 2^-24):
(a) every kernel: |kernel - float64 reference| within a bound worked out from the operation count --
    maps (C+1) u sum_c|g_c| / C; normalised accumulate 2 groups u max_s|v/m| + 1e-15 |ref|; trapezoid
    over K total steps (K+2) u sum_k|G_k|; weighted (groups+1) u sum|w_s G_s|; cube mode 0 (n_total
    >= 2) 4 u max(|acc0|, max|v|); fp64 accumulators and k_reproject 1e-12 relative. The trapezoid
    and weighted chains start from a zero accumulator (later passes carry a non-zero acc and prev),
    so every partial sum is at most sum|G| and K adds of u/2 each stay inside the bound.
(b) where the contract is a fixed sequence of fp32 adds and divisions without a multiply-add:
    equality, bit for bit, with the fp32-emulated reference. Pixels fed +-inf are judged by (b) only
    (FLT_MAX + FLT_MAX overflows in fp32, not in float64).
The largest error / bound ratio per kernel is printed when the module finishes.
"""
import numpy as np
import pytest
import torch

from tests import epilogue_ref as R

pytestmark = pytest.mark.gpu
U = R.U
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def P():
    from wam_amd import plan
    assert torch.cuda.is_available()
    yield plan
    torch.cuda.synchronize()
    for k in sorted(R.WORST):
        print("[epilogue] worst error / bound of %s = %.3g" % (k, R.WORST[k]))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


# ------------------------------------------------------------------------------ maps
MAP_PLANS = {
    "db4_37x53_J2": (2, (37, 53), 2, "db4"),      # bands of 252 and 660 below one 8,192 tile: 16-byte path
    "db4_37x51_J2": (2, (37, 51), 2, "db4"),      # bands of 638 (no multiple of 4) below one tile: scalar path
    "haar_200_J1": (2, (200, 200), 1, "haar"),    # bands of 10,000: a partial second tile, 16-byte path
    "db4_224_J1": (2, (224, 224), 1, "db4"),      # bands of 13,225: a second tile on the scalar path
    "db2_1d_1000_J3": (1, (1000,), 3, "db2"),
}


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("name", list(MAP_PLANS))
def test_subband_maps(P, name, C):
    """wam_subband_maps vs maps_ref, 3 groups x 2 items, a NaN in one item of group 1: (a), (b), and
    band_max NaN at exactly (group 1, that band). Previously unreached branch 6: k_subband_maps with
    a band longer than one 8,192-element tile on the 16-byte path (haar 200^2) and on the scalar path
    (db4 224^2), the NaN in the band's LAST element (the partial second tile), so the group boundary
    of band_max is crossed with NaN in one group only. Below one tile: db4 (37, 53) J=2 has bands of
    252 and 660, all multiples of 4 (the 16-byte path); the scalar path below one tile is db4
    (37, 51) J=2 with bands of 638. want_max=False: the same maps, no maxima."""
    ndim, shape, J, wav = MAP_PLANS[name]
    p = P.get_plan(ndim, shape, J, wav, "reflect", "cuda")
    off = list(p.band_offsets)
    sizes = np.diff(off)
    if name == "haar_200_J1":
        assert sizes.max() == 10000 and all(o % 4 == 0 for o in off)
    if name == "db4_224_J1":
        assert sizes.max() == 13225
    if name == "db4_37x53_J2":
        assert sizes.max() < 8192 and all(o % 4 == 0 for o in off)
    if name == "db4_37x51_J2":
        assert sizes.max() == 638 and any(o % 4 for o in off)
    groups, gi = 3, 2
    items = groups * gi
    rng = np.random.RandomState(17 + C)
    g = rng.standard_normal(items * C * off[-1]).astype(F32)
    # distinct scale per item so that the maximum of another group is a different number
    bnan = p.nbands - 1
    for b in range(p.nbands):
        blk = g[items * C * off[b]:items * C * off[b + 1]].reshape(items, C, -1)
        blk *= (1.5 ** np.arange(items, dtype=F32))[:, None, None]
    blk = g[items * C * off[bnan]:items * C * off[bnan + 1]].reshape(items, C, -1)
    blk[gi + 1, C - 1, -1] = np.nan   # group 1, its second item, last channel, last element
    maps, bmax = P.subband_maps(p, dev(g), groups, gi, C)
    maps, bmax = host(maps).reshape(items, -1), host(bmax)
    r64, b64 = R.maps_ref(g, groups, gi, C, off)
    r32, b32 = R.maps_ref(g, groups, gi, C, off, dt=F32)
    bound = (C + 1) * U * R.maps_abs_sum(g, items, C, off) / C
    R.assert_within(maps, r64, bound, "maps %s C=%d" % (name, C))
    R.assert_bits(maps, r32, "maps %s C=%d" % (name, C))
    R.assert_bits(bmax, b32, "band_max %s C=%d" % (name, C))
    want_nan = np.zeros((groups, p.nbands), dtype=bool)
    want_nan[1, bnan] = True
    assert np.array_equal(np.isnan(bmax), want_nan)
    assert np.array_equal(np.isnan(b64), want_nan) and np.isfinite(bmax[~want_nan]).all()
    m2, none = P.subband_maps(p, dev(g), groups, gi, C, want_max=False)
    assert none is None
    R.assert_bits(host(m2).reshape(items, -1), r32, "maps(want_max=False) %s C=%d" % (name, C))


# ------------------------------------------------------------------------------ mosaic frames
class Mosaic:
    """Synthetic injective tables and per-pass maps: `passes` chained groups of n items; band maxima
    distinct per (group, band) by factors of 1.5; band 2 of the last group of every pass all zero
    with zero maximum; a NaN map value and inf at a fixed handful of (step, coefficient) positions."""

    def __init__(self, seed, n, F, K, nb, mapped, passes, specials=True):
        rng = np.random.RandomState(seed)
        self.n, self.F, self.K, self.nb, self.passes = n, F, K, nb, passes
        self.src, self.band, self.dst, self.cband = R.make_tables(rng, F, K, nb, mapped)
        G = sum(passes)
        self.bmax = (0.5 * 1.5 ** (np.arange(G * nb) % 23).reshape(G, nb)).astype(F32)
        self.maps = rng.uniform(0.1, 1.0, (G * n, K)).astype(F32) * np.repeat(self.bmax, n, axis=0)[:, self.cband]
        self.inf_mask = np.zeros((n, F), dtype=bool)
        valid = np.flatnonzero(self.src >= 0)
        self.zero_pix = (self.src >= 0) & (self.band == 2)
        if specials:
            k = 0
            for g in passes:
                k += g
                self.maps[(k - 1) * n:k * n, self.cband == 2] = 0.0
                self.bmax[k - 1, 2] = 0.0
            ok = valid[self.band[valid] != 2]
            self.maps[0 * n + 1, self.src[ok[3]]] = np.nan   # step 0, item 1
            # inf: (step, item, pixel); the first two are consecutive steps of one pixel where
            # the chain allows (FLT_MAX + FLT_MAX overflows in fp32)
            for step, item, pix in ((min(1, G - 1), 0, ok[5]), (min(2, G - 1), 0, ok[5]), (G - 1, n - 1, ok[9]),
                                    (0, 2 % n, ok[11])):
                self.maps[step * n + item, self.src[pix]] = np.inf
                self.inf_mask[item, pix] = True
        self.weights = (rng.uniform(0.5, 1.5, G) * (1.0 + np.arange(G) % 5)).astype(F32)
        self.d = {k: dev(getattr(self, k)) for k in ("src", "band", "dst", "cband")}

    def slices(self):
        k0 = 0
        for g in self.passes:
            yield g, k0, self.maps[k0 * self.n:(k0 + g) * self.n], self.bmax[k0:k0 + g], self.weights[k0:k0 + g]
            k0 += g

    def steps(self, normalize):
        """G[k, n, p] (float64, after nan_to_num) of the whole chain -- the scale of the bounds"""
        out = []
        for g, _, maps, bmax, _ in self.slices():
            for s in range(g):
                valid, v = R._mosaic_values(maps, bmax, self.src, self.band, s, self.n, normalize, F64)
                G = np.zeros((self.n, self.F))
                G[:, valid] = R._nan_to_num(v)
                out.append(G)
        return np.stack(out)


def _accumulate(P, form, m, g, maps, bmax, normalize, frame):
    from wam_amd._lib import check, lib, ptr, stream_of
    st = stream_of(frame.device)
    if form == "coef":
        check(lib.wam_frame_accumulate_coef(g, m.n, m.K, m.F, ptr(m.d["dst"]), ptr(m.d["cband"]), ptr(maps), ptr(bmax),
                                            m.nb, int(normalize), ptr(frame), st))
    else:
        check(lib.wam_frame_accumulate(g, m.n, m.F, ptr(m.d["src"]), ptr(m.d["band"]), ptr(maps), m.K, ptr(bmax), m.nb,
                                       int(normalize), ptr(frame), st))


def _trapz(P, form, m, g, k0, maps, bmax, normalize, w, prev, acc):
    from wam_amd._lib import check, lib, ptr, stream_of
    st = stream_of(acc.device)
    if form == "coef":
        check(lib.wam_frame_trapz_coef(g, k0, m.n, m.K, m.F, ptr(m.d["dst"]), ptr(m.d["cband"]), ptr(maps), ptr(bmax),
                                       m.nb, int(normalize), ptr(w), ptr(prev), ptr(acc), st))
    else:
        check(lib.wam_frame_trapz(g, k0, m.n, m.F, ptr(m.d["src"]), ptr(m.d["band"]), ptr(maps), m.K, ptr(bmax), m.nb,
                                  int(normalize), ptr(w), ptr(prev), ptr(acc), st))


def _check_accumulate(P, form, m, normalize, tag):
    rng = np.random.RandomState(3)
    frame0 = rng.standard_normal((m.n, m.F))
    fr = dev(frame0)
    r64 = r32 = frame0
    vmax = np.zeros((m.n, m.F))
    for g, _, maps, bmax, _ in m.slices():
        _accumulate(P, form, m, g, dev(maps), dev(bmax), normalize, fr)
        r64 = R.frame_accumulate_ref(r64, maps, bmax, m.src, m.band, g, m.n, normalize)
        r32 = R.frame_accumulate_ref(r32, maps, bmax, m.src, m.band, g, m.n, normalize, emulate=True)
        for s in range(g):
            valid, v = R._mosaic_values(maps, bmax, m.src, m.band, s, m.n, normalize, F64)
            vmax[:, valid] = np.fmax(vmax[:, valid], np.where(np.isfinite(v), np.abs(v), 0.0))
    got = host(fr)
    G = sum(m.passes)
    bound = 2 * G * U * vmax + 1e-15 * np.abs(np.nan_to_num(r64)) if normalize else R.rel_bound(r64[np.isfinite(r64)])
    R.assert_within(got, r64, bound, "frame_accumulate%s %s" % ("" if normalize else "(raw)", tag),
                    exclude=m.inf_mask if m.inf_mask.any() else None)
    # the contract's own order: fp32 quotient widened, fp64 sum in group order (inf pixels included)
    R.assert_bits(got, r32, "frame_accumulate %s" % tag)
    assert np.array_equal(got[:, m.src < 0], frame0[:, m.src < 0])
    return got


@pytest.mark.parametrize("groups", [1, 8, 11])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("form", ["pixel", "coef"])
def test_frame_accumulate(P, form, normalize, groups):
    """wam_frame_accumulate (pixel order) and wam_frame_accumulate_coef (coefficient order) vs
    frame_accumulate_ref: 3 items, frame_len 1,203 and maps_item_len 1,231 (no multiples of 256),
    groups of 1, 8 and 11 (the block-of-8 loop and its tail), a non-zero incoming frame, holes
    untouched. The all-zero band with zero maximum gives NaN at exactly the reference's pixels when
    normalised (SmoothGrad's 0 / 0)."""
    m = Mosaic(100 + groups, 3, 1203, 1231, 5, 1000, (groups,))
    got = _check_accumulate(P, form, m, normalize, "%s g=%d" % (form, groups))
    if normalize:
        assert np.isnan(got[:, m.zero_pix]).all() and m.zero_pix.sum() > 20
    else:
        assert np.isnan(got).sum() == 1


@pytest.mark.parametrize("groups", [1, 8, 11])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("form", ["pixel", "coef"])
def test_frame_trapz_sequential(P, form, normalize, groups):
    """wam_frame_trapz / wam_frame_trapz_coef, sequential: three chained passes (groups, 2, groups)
    carrying prev and k0 vs frame_trapz_ref -- (a) over the K total steps, (b) on every pixel, the
    inf-fed ones included. The all-zero band gives 0 after nan_to_num (IG), the NaN map value 0."""
    m = Mosaic(200 + groups, 3, 1203, 1231, 5, 1000, (groups, 2, groups))
    prev, acc = dev(np.zeros((m.n, m.F), F32)), dev(np.zeros((m.n, m.F), F32))
    p64 = a64 = np.zeros((m.n, m.F))
    p32 = a32 = np.zeros((m.n, m.F), F32)
    for g, k0, maps, bmax, _ in m.slices():
        _trapz(P, form, m, g, k0, dev(maps), dev(bmax), normalize, None, prev, acc)
        p64, a64 = R.frame_trapz_ref(p64, a64, maps, bmax, m.src, m.band, g, k0, m.n, normalize)
        p32, a32 = R.frame_trapz_ref(p32, a32, maps, bmax, m.src, m.band, g, k0, m.n, normalize, dt=F32)
    G = m.steps(normalize)
    K = G.shape[0]
    tag = "%s norm=%d g=%d" % (form, normalize, groups)
    R.assert_within(host(acc), a64, (K + 2) * U * np.abs(G).sum(axis=0), "frame_trapz " + tag, exclude=m.inf_mask)
    R.assert_bits(host(acc), a32, "frame_trapz acc " + tag)
    R.assert_bits(host(prev), p32, "frame_trapz prev " + tag)
    assert not np.isnan(host(acc)).any()
    if normalize:  # the 0 / 0 steps count as 0: those pixels hold the trapezoid of the other steps
        assert np.isfinite(host(acc)[:, m.zero_pix]).all() and (host(prev)[:, m.zero_pix] == 0).all()


@pytest.mark.parametrize("groups", [1, 8, 11])
@pytest.mark.parametrize("form", ["pixel", "coef"])
def test_frame_trapz_weighted(P, form, groups):
    """weighted mode (acc += w[s] * G, distinct weights), two chained passes, normalised: (a) only --
    the kernel uses a fused multiply-add, which the contract leaves open. prev is not touched."""
    m = Mosaic(300 + groups, 3, 1203, 1231, 5, 1000, (groups, groups))
    prev0 = np.random.RandomState(1).uniform(0.5, 1, (m.n, m.F)).astype(F32)
    prev, acc = dev(prev0), dev(np.zeros((m.n, m.F), F32))
    a64 = np.zeros((m.n, m.F))
    for g, k0, maps, bmax, w in m.slices():
        _trapz(P, form, m, g, k0, dev(maps), dev(bmax), True, dev(w), prev, acc)
        _, a64 = R.frame_trapz_ref(prev0, a64, maps, bmax, m.src, m.band, g, k0, m.n, True, weights=w)
    G = m.steps(True)
    bound = (G.shape[0] + 1) * U * (np.abs(G) * m.weights.astype(F64)[:, None, None]).sum(axis=0)
    R.assert_within(host(acc), a64, bound, "frame_trapz_weighted %s g=%d" % (form, groups), exclude=m.inf_mask)
    assert np.array_equal(host(prev), prev0)


def test_frame_coef_runs_branches(P):
    """Previously unreached branch 2: the runs-of-items branch (items_per_thread > 1) of
    k_frame_accumulate_coef -- maps_item_len 262,200 (tables over 2 MB), 9 items: 2 items per thread
    and a partial last run -- and the trapezoid's with a partial last run (33 items: 2 per thread, 17
    runs). 2 groups; the trapezoid runs at k0 = 3 from a non-zero prev (the value of step 2, part of
    the K = 3 values of the bound)."""
    K, F = 262200, 262400
    m = Mosaic(7, 9, F, K, 5, 200000, (2,))
    _check_accumulate(P, "coef", m, True, "coef runs 9 items")
    m = Mosaic(8, 33, F, K, 5, 200000, (2,), specials=False)
    rng = np.random.RandomState(2)
    prev0 = rng.uniform(0.1, 1, (m.n, F)).astype(F32)
    prev0[:, m.src < 0] = 0
    prev, acc = dev(prev0), dev(np.zeros((m.n, F), F32))
    _trapz(P, "coef", m, 2, 3, dev(m.maps), dev(m.bmax), True, None, prev, acc)
    p64, a64 = R.frame_trapz_ref(prev0, np.zeros((m.n, F)), m.maps, m.bmax, m.src, m.band, 2, 3, m.n, True)
    p32, a32 = R.frame_trapz_ref(prev0, np.zeros((m.n, F), F32), m.maps, m.bmax, m.src, m.band, 2, 3, m.n, True, dt=F32)
    scale = np.abs(prev0.astype(F64)) + np.abs(m.steps(True)).sum(axis=0)
    R.assert_within(host(acc), a64, (3 + 2) * U * scale, "frame_trapz coef runs 33 items")
    R.assert_bits(host(acc), a32, "frame_trapz coef runs acc")
    R.assert_bits(host(prev), p32, "frame_trapz coef runs prev")


# ------------------------------------------------------------------------------ cube
CUBES = {"strided_256x3": (256, 3), "strided_span_384x2": (384, 2), "consecutive_252x3": (252, 3), "scalar_253x3": (253, 3)}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(CUBES))
def test_cube_accumulate(P, name, mode):
    """wam_cube_accumulate vs cube_ref, two chained passes (3 and 5 groups: the 4-sample gather
    blocks and their tail), holes in src, signed values; prev=None in modes 0 and 1; mode 2 with NaN
    / inf values and a random incoming prev that k0 = 0 must ignore. Previously unreached branch 1:
    k_cube_accumulate4<STRIDED> with a 256-voxel wave block that spans two items (cube_len 384 with
    2 items: the work is 3 x 256, block 1 covers voxels 256..383 of item 0 and 0..127 of item 1).
    cube_len 256 x 3: strided; 252: four consecutive voxels; 253: the one-voxel kernel."""
    L, n = CUBES[name]
    K = L + 37
    rng = np.random.RandomState(L + mode)
    src = rng.permutation(K)[:L].astype(np.int32)
    src[::13] = -1
    passes = (3, 5)
    maps = [rng.standard_normal((g * n, K)).astype(F32) for g in passes]
    inf_mask = np.zeros((n, L), dtype=bool)
    if mode == 2:
        maps[0][0 * n + 0, src[1]] = np.nan
        for step, pix in ((1, 2), (2, 2), (0, 5)):   # two consecutive inf steps at voxel 2 of the last item
            maps[0][step * n + n - 1, src[pix]] = np.inf
            inf_mask[n - 1, pix] = True
        maps[1][4 * n, src[7]] = -np.inf
        inf_mask[0, 7] = True
    ws = [(rng.uniform(0.5, 1.5, g) * (1 + np.arange(g))).astype(F32) for g in passes]
    acc0 = rng.uniform(0.5, 1.0, (n, L)).astype(F32) if mode == 0 else np.zeros((n, L), F32)
    prev0 = rng.uniform(0.5, 1.0, (n, L)).astype(F32) if mode == 2 else None
    acc, prev, dsrc = dev(acc0), dev(prev0), dev(src)
    assert dsrc.data_ptr() % 16 == 0 and acc.data_ptr() % 16 == 0
    p64, a64, p32, a32 = prev0, acc0, prev0, acc0
    k0 = 0
    for g, mp, w in zip(passes, maps, ws):
        P.cube_accumulate(g, k0, n, dsrc, dev(mp), K, mode, 25.0, acc, prev=prev, weights=dev(w) if mode == 1 else None)
        p64, a64 = R.cube_ref(p64, a64, mp, src, g, k0, n, mode, 25.0, w)
        p32, a32 = R.cube_ref(p32, a32, mp, src, g, k0, n, mode, 25.0, w, dt=F32)
        k0 += g
    valid = src >= 0
    V = np.zeros((sum(passes), n, L))      # the value of every (step, item, voxel)
    V[:, :, valid] = np.concatenate([mp.reshape(g, n, K) for g, mp in zip(passes, maps)])[:, :, src[valid]]
    V = R._nan_to_num(V) if mode == 2 else V
    if mode == 0:
        bound = 4 * U * np.maximum(np.abs(acc0), np.abs(V).max(axis=0))
    elif mode == 1:
        bound = (V.shape[0] + 1) * U * (np.abs(V) * np.concatenate(ws).astype(F64)[:, None, None]).sum(axis=0)
    else:
        bound = (V.shape[0] + 2) * U * np.abs(V).sum(axis=0)
    tag = "%s mode %d" % (name, mode)
    R.assert_within(host(acc), a64, bound, "cube_accumulate " + tag, exclude=inf_mask if mode == 2 else None,
                    max_excluded=0.01)
    if mode != 1:
        R.assert_bits(host(acc), a32, "cube_accumulate acc " + tag)
    if mode == 2:
        R.assert_bits(host(prev), p32, "cube_accumulate prev " + tag)


# ------------------------------------------------------------------------------ fp32 streams
@pytest.mark.parametrize("scale", [0.0, 25.0])
@pytest.mark.parametrize("groups", [1, 7])
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_accumulate_f32(P, n, groups, scale):
    """Previously unreached entry 7: wam_accumulate_f32 on its own, with a non-zero incoming acc that
    `scale` must divide too. Bound: groups adds and one division, (groups + 1) u (|acc0| + sum|src|)
    / scale."""
    rng = np.random.RandomState(n + groups)
    src = rng.standard_normal((groups, n)).astype(F32)
    acc0 = rng.uniform(0.5, 1.0, n).astype(F32)
    acc = dev(acc0)
    P.accumulate_f32(dev(src), groups, acc, scale)
    bound = (groups + 1) * U * (np.abs(acc0) + np.abs(src).sum(axis=0)) / (scale or 1.0)
    tag = "n=%d g=%d scale=%g" % (n, groups, scale)
    R.assert_within(host(acc), R.accumulate_ref(acc0, src, groups, scale), bound, "accumulate_f32 " + tag)
    R.assert_bits(host(acc), R.accumulate_ref(acc0, src, groups, scale, dt=F32), "accumulate_f32 " + tag)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("groups", [1, 7])
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_trapz_f32(P, n, groups, f64):
    """Previously unreached entry 7: wam_trapz_f32 on its own -- fp32 and fp64 accumulators, two
    chained sequential passes (a k0 carry through prev), and weights with prev=None. fp32
    sequential: (a) and (b); fp32 weighted: (a); fp64: 1e-12 relative."""
    rng = np.random.RandomState(n + groups)
    dt, tdt = (F64, torch.float64) if f64 else (F32, torch.float32)
    srcs = [rng.standard_normal((groups, n)).astype(F32) for _ in range(2)]
    ws = [(rng.uniform(0.5, 1.5, groups) * (1 + np.arange(groups))).astype(F32) for _ in range(2)]
    tag = "n=%d g=%d %s" % (n, groups, "f64" if f64 else "f32")
    # sequential
    prev, acc = torch.zeros(n, dtype=tdt, device="cuda"), torch.zeros(n, dtype=tdt, device="cuda")
    p64 = a64 = np.zeros(n)
    p32 = a32 = np.zeros(n, F32)
    for i, s in enumerate(srcs):
        P.trapz_stream(dev(s), groups, i * groups, prev, acc)
        p64, a64 = R.trapz_stream_ref(p64, a64, s, groups, i * groups)
        p32, a32 = R.trapz_stream_ref(p32, a32, s, groups, i * groups, dt=F32)
    allsrc = np.abs(np.concatenate(srcs).astype(F64))
    if f64:
        R.assert_within(host(acc), a64, R.rel_bound(a64), "trapz_f64 " + tag)
        assert np.array_equal(host(prev), p64)
    else:
        R.assert_within(host(acc), a64, (2 * groups + 2) * U * allsrc.sum(axis=0), "trapz_f32 " + tag)
        R.assert_bits(host(acc), a32, "trapz_f32 acc " + tag)
        R.assert_bits(host(prev), p32, "trapz_f32 prev " + tag)
    # weighted, prev=None
    acc = torch.zeros(n, dtype=tdt, device="cuda")
    a64 = np.zeros(n)
    for s, w in zip(srcs, ws):
        P.trapz_stream(dev(s), groups, 0, None, acc, weights=dev(w))
        _, a64 = R.trapz_stream_ref(None, a64, s, groups, 0, weights=w)
    if f64:
        R.assert_within(host(acc), a64, R.rel_bound(a64), "trapz_f64_weighted " + tag)
    else:
        bound = (2 * groups + 1) * U * (allsrc * np.concatenate(ws).astype(F64)[:, None]).sum(axis=0)
        R.assert_within(host(acc), a64, bound, "trapz_f32_weighted " + tag)


# ------------------------------------------------------------------------------ refusals
def test_argument_errors_launch_nothing(P):
    """The host checks of the seven accumulator entries, on 2 items, a frame of 5 pixels, 7
    coefficients, 2 bands, 2 groups: every required pointer NULL in turn, every checked count
    negative, normalize without band_max, the cube's mode 3 / mode 1 without weights / mode 2 without
    prev, wam_trapz_f32 without an accumulator or sequential without the accumulator's own prev all
    return WAM_ERR_INVALID_ARG; zero groups and zero work return WAM_OK; and no output buffer
    (filled with 7) changes a bit. Valid arguments would change them: the maps are all ones."""
    from wam_amd._lib import lib, ptr, stream_of
    OK, INVALID = 0, 1
    n, F, K, nb, G = 2, 5, 7, 2, 2
    i32 = lambda *v: dev(np.array(v, np.int32))
    src, band = i32(3, -1, 0, 6, 2), i32(1, 0, 0, 1, 0)                     # pixel -> coefficient, its band
    dst, cband = i32(2, -1, 4, 0, -1, -1, 3), i32(0, 0, 0, 1, 1, 1, 1)      # the same mosaic, coefficient -> pixel
    ones = lambda *shape: torch.ones(shape, device="cuda")
    maps, bmax, w, stream = ones(G * n, K), ones(G, nb), ones(G), ones(G, n * F)
    outs = {k: torch.full((n * F,), 7.0, dtype=dt, device="cuda")
            for k, dt in (("frame", torch.float64), ("prev", torch.float32), ("acc", torch.float32),
                          ("prev64", torch.float64), ("acc64", torch.float64))}
    st = stream_of(maps.device)

    def entry(fn, order, **defaults):
        def call(**kw):
            a = dict(defaults, **kw)
            return fn(*[a[k] if isinstance(a[k], (int, float)) else ptr(a[k]) for k in order.split()], st)
        return call

    pix = dict(groups=G, k0=0, n=n, F=F, src=src, band=band, maps=maps, K=K, bmax=bmax, nb=nb, norm=1, w=None, **outs)
    coef = dict(pix, dst=dst, cband=cband)
    cube = dict(groups=G, k0=0, n=n, L=F, src=src, maps=maps, K=K, mode=2, n_total=25.0, w=w, **outs)
    flat = dict(groups=G, k0=0, len=n * F, src=stream, scale=25.0, w=None, **outs)
    # entry, its required pointers, its checked counts, further refusals, calls with nothing to do
    table = [
        (entry(lib.wam_frame_accumulate, "groups n F src band maps K bmax nb norm frame", **pix),
         "src band maps frame", "groups n F", [{"bmax": None}], [{"groups": 0}, {"n": 0}, {"F": 0}]),
        (entry(lib.wam_frame_accumulate_coef, "groups n K F dst cband maps bmax nb norm frame", **coef),
         "dst cband maps frame", "groups n K F", [{"bmax": None}], [{"groups": 0}, {"n": 0}, {"K": 0}]),
        (entry(lib.wam_frame_trapz, "groups k0 n F src band maps K bmax nb norm w prev acc", **pix),
         "src band maps prev acc", "groups n F", [{"bmax": None}, {"bmax": None, "w": w}],
         [{"groups": 0}, {"n": 0}, {"F": 0}]),
        (entry(lib.wam_frame_trapz_coef, "groups k0 n K F dst cband maps bmax nb norm w prev acc", **coef),
         "dst cband maps prev acc", "groups n K F", [{"bmax": None}, {"bmax": None, "w": w}],
         [{"groups": 0}, {"n": 0}, {"K": 0}]),
        (entry(lib.wam_cube_accumulate, "groups k0 n L src maps K mode n_total w prev acc", **cube),
         "src maps acc", "groups n L", [{"mode": 3}, {"mode": -1}, {"mode": 1, "w": None}, {"mode": 2, "prev": None}],
         [{"groups": 0}, {"n": 0}, {"L": 0}, {"groups": 0, "mode": 0, "prev": None}]),
        (entry(lib.wam_accumulate_f32, "groups len src scale acc", **flat),
         "src acc", "groups len", [], [{"len": 0}, {"groups": 0, "scale": 0.0}]),   # no groups: acc / scale alone
        (entry(lib.wam_trapz_f32, "groups k0 len src w prev acc prev64 acc64", **flat),
         "src", "groups len", [{"acc": None, "acc64": None}, {"prev": None, "acc64": None}, {"prev64": None},
                               {"acc": None, "prev": None, "prev64": None}],
         [{"len": 0}, {"groups": 0}, {"len": 0, "acc64": None}, {"groups": 0, "w": w, "prev": None, "prev64": None}]),
    ]
    for call, pointers, counts, refused, nothing in table:
        for kw in [{k: None} for k in pointers.split()] + [{k: -1} for k in counts.split()] + refused:
            assert call(**kw) == INVALID, kw
        for kw in nothing:
            assert call(**kw) == OK, kw
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == 7.0).all()), k


# ------------------------------------------------------------------------------ sigma
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("items,stride,length", [(3, 1001, 999), (5, 4096, 4096), (1, 7, 7), (2, 40000, 37),
                                                 (4, 20000, 20000)])
def test_item_sigma_one_block_per_item(P, items, stride, length, offset):
    """Previously unreached entry 3: wam_item_sigma, the one-block-per-item form (the Python layer
    only calls wam_item_sigma_ws), through _lib: spread * (max - min) in fp32 as
    test_item_sigma_split_matches_torch states it, ragged / constant-item / NaN-item cases; offset 1
    hands over a pointer 4 bytes off 16-byte alignment (the scalar path); (4, 20000) runs the
    16-byte path's 4-load loop."""
    from wam_amd._lib import check, lib, ptr, stream_of
    torch.manual_seed(23)
    buf = torch.randn(items * stride + 4, device="cuda") * 3.0
    x = buf[offset:offset + items * stride]
    assert (x.data_ptr() % 16 == 0) == (offset == 0)
    xv = x.view(items, stride)[:, :length]
    if items >= 3:
        xv[1].fill_(0.75)                     # constant item
        xv[2, length // 2] = float("nan")     # NaN item
    spread = 0.15
    got = torch.empty(items, device="cuda")
    check(lib.wam_item_sigma(items, stride, length, ptr(x), float(np.float32(spread)), ptr(got), stream_of(x.device)))
    ref = np.float32(spread) * (xv.amax(dim=1) - xv.amin(dim=1))
    if items >= 3:
        assert torch.isnan(got[2]) and torch.isnan(ref[2])
        assert float(got[1]) == 0.0
    ok = ~torch.isnan(ref)
    assert torch.equal(got[ok], ref[ok])
    R.assert_bits(host(got), R.sigma_ref(host(x), items, stride, length, spread), "item_sigma")
    assert torch.equal(P.item_sigma(x, stride, length, spread)[ok], got[ok])


# ------------------------------------------------------------------------------ .scales
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("size,levels", [(8, 1), (8, 3), (20, 3), (37, 2), (37, 4), (64, 5), (12, 3)])
def test_reproject_scales(P, size, levels, approx):
    """wam_reproject_scales (float64) vs reproject_ref at 1e-12 relative, 2 items. Previously
    unreached branch 5: sizes not divisible by 2^levels -- (20, 3), (37, 2), (37, 4), (12, 3) -- take
    the int(size / 2**j) splits."""
    avg = np.random.RandomState(size + levels).standard_normal((2, size, size))
    got = host(P.reproject_scales(dev(avg), levels, approx))
    ref = R.reproject_ref(avg, levels, approx)
    R.assert_within(got, ref, R.rel_bound(ref), "reproject %d/%d approx=%d" % (size, levels, approx))


def test_reproject_scales_plane_wrap(P):
    """Previously unreached branch 4: k_reproject's `q += gridDim.y` wrap -- size 4, levels 2 with
    the approximation, 21,846 items: 65,538 output planes over a 65,535-row grid (8 MB of output)."""
    items = 21846
    avg = np.random.RandomState(0).standard_normal((items, 4, 4))
    got = host(P.reproject_scales(dev(avg), 2, True))
    ref = R.reproject_ref(avg, 2, True)
    assert got.shape == (items, 3, 4, 4) and items * 3 > 65535
    R.assert_within(got, ref, R.rel_bound(ref), "reproject wrap")
    assert np.abs(got[-1]).min() > 0  # the wrapped planes were written


@pytest.mark.parametrize("size,levels", [(4, 3), (6, 3), (3, 2)])
def test_reproject_scales_refuses_empty_quadrant(P, size, levels):
    """size < 2^levels: WAM_ERR_INVALID_ARG before any launch (the reference raises on the empty
    quadrant). Only the return code is looked at; nothing runs on that input."""
    from wam_amd._lib import WamError, lib, ptr, stream_of
    avg = torch.ones((1, size, size), dtype=torch.float64, device="cuda")
    out = torch.zeros((1, levels + 1, size, size), dtype=torch.float64, device="cuda")
    for approx in (0, 1):
        assert lib.wam_reproject_scales(1, size, levels, approx, ptr(avg), ptr(out), stream_of(avg.device)) == 1
    with pytest.raises(WamError):
        P.reproject_scales(avg, levels, True)
    assert not out.any()


def test_set_result_leaves_scales_unset_below_2_pow_J(P):
    """get_plan admits geometries smaller than 2^J (a 4 x 4 haar J=3 plan is created), so
    WaveletAttribution2D._set_result must not fail the call that produced such a map: it leaves
    _scales_res unset and .scales raises ValueError, as the reference raises when it builds them.
    An 8 x 8 map still gets its scales inside the call."""
    from wam_amd.wam_2D import WaveletAttribution2D
    ex = WaveletAttribution2D(torch.nn.Conv2d(3, 1, 1).cuda(), wavelet="haar", J=3, approx_coeffs=True)
    ex._set_result(torch.ones((1, 4, 4), dtype=torch.float64, device="cuda"))
    assert ex._scales_res is None
    with pytest.raises(ValueError):
        ex.scales
    avg = np.random.RandomState(1).standard_normal((2, 8, 8))
    ex._set_result(dev(avg))
    assert ex._scales_res is not None
    ref = R.reproject_ref(avg, 3, True)
    R.assert_within(ex.scales, ref, R.rel_bound(ref), "reproject via _set_result")


@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("items", [1, 3])
@pytest.mark.parametrize("wav,J,side", [("db4", 2, 37), ("haar", 3, 40)])
def test_disentangle_scales_vs_oracle(P, wav, J, side, items, C, approx):
    """plan.disentangle_scales on random packed gradients (through wam_subband_maps, one group) vs
    oracle.wam_ref.disentangle_scales_2d at the 1e-5 of the golden test; with approx the
    approximation row belongs to the LAST item only."""
    from oracle import wam_ref
    p = P.get_plan(2, (side, side), J, wav, "reflect", "cuda")
    rng = np.random.RandomState(items + 10 * C)
    bands = [rng.standard_normal((items, C) + tuple(s)).astype(F32) for s in p.band_shapes]
    g = np.concatenate([b.reshape(-1) for b in bands])
    maps, bmax = P.subband_maps(p, dev(g), 1, items, C)
    size = 2 * p.band_shapes[-1][1]
    got = host(P.disentangle_scales(p, maps, bmax, items, approx, size))
    grads = [bands[0]] + [tuple(bands[1 + 3 * l:4 + 3 * l]) for l in range(J)]
    ref = wam_ref.disentangle_scales_2d(grads, J, approx)
    R.assert_within(got, ref, 1e-5, "disentangle %s J=%d n=%d C=%d approx=%d" % (wav, J, items, C, approx))
    if approx and items > 1:
        assert not got[:-1, J].any() and np.abs(got[-1, J]).max() > 0.1
