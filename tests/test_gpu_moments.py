"""SmoothGrad-squared / VarGrad: the moment entries of include/wam_hip.h at the C
ABI, bit for bit against numpy float64 loops in sample order, and the 'smooth_sq' / 'vargrad' methods of
the three attribution classes against the CPU restatement tests/moments_ref.py.

Why bits at the C ABI: S += fp64(v) and Q += fp64(v) * fp64(v) are one float64 add each per sample (the
product of two widened float32 values is exact), so a numpy float64 loop in the same order is the
contract itself. Class bars: the suite holds a per-sample map to 1e-4 (absolute for the normalised 2D
mosaic with v in [0, 1], relative to the maximum for the raw 1D / 3D gradients); with |dv| <= delta,
|d(v^2)| <= 2 delta and |d(m^2)| <= 2 delta, so 2e-4 for smooth_sq and 4e-4 for vargrad.
"""
import numpy as np
import pytest
import torch

import testmodels
from tests import moments_ref as M

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OK, INVALID = 0, 1


@pytest.fixture(scope="module")
def P():
    from wam_amd import plan
    assert torch.cuda.is_available()
    return plan


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def zeros64(*shape):
    return torch.zeros(shape, dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------ 2D mosaic
PLANS_2D = {"haar_J2_16x16": ((16, 16), 2, "haar"), "db4_J2_20x24": ((20, 24), 2, "db4")}


class Frame2D:
    """A plan's native-frame mosaic in both orders and random maps / band maxima of `groups` x 2 items."""

    def __init__(self, P, name, groups, seed):
        from wam_amd import frames
        shape, J, wav = PLANS_2D[name]
        self.p = P.get_plan(2, shape, J, wav, "reflect", "cuda")
        self.n, self.groups, self.K, self.nb = 2, groups, self.p.coeff_numel, self.p.nbands
        self.gmap, (h, w) = frames.smooth_frame(self.p, self.n, "native", torch.device("cuda", torch.cuda.current_device()))
        self.F = h * w
        self.inv = P._inverse_map(self.gmap, self.K)
        assert self.inv is not None
        self.src, self.band = host(self.gmap[0]), host(self.gmap[1])
        rng = np.random.RandomState(seed)
        self.bmax = (0.5 * 1.5 ** (rng.permutation(groups * self.nb) % 7).reshape(groups, self.nb)).astype(F32)
        self.maps = rng.uniform(0.05, 1.0, (groups * self.n, self.K)).astype(F32)

    def run(self, form, normalize, S, Q, g0=0, g=None):
        from wam_amd._lib import check, lib, ptr, stream_of
        g = self.groups - g0 if g is None else g
        maps, bmax = dev(self.maps[g0 * self.n:(g0 + g) * self.n]), dev(self.bmax[g0:g0 + g])
        st = stream_of(S.device)
        if form == "coef":
            check(lib.wam_frame_moments_coef(g, self.n, self.K, self.F, ptr(self.inv[0]), ptr(self.inv[1]), ptr(maps),
                                             ptr(bmax), self.nb, int(normalize), ptr(S), ptr(Q), st))
        elif form == "pixel":
            check(lib.wam_frame_moments(g, self.n, self.F, ptr(self.gmap[0]), ptr(self.gmap[1]), ptr(maps), self.K,
                                        ptr(bmax), self.nb, int(normalize), ptr(S), ptr(Q), st))
        else:  # the existing single sum
            check(lib.wam_frame_accumulate_coef(g, self.n, self.K, self.F, ptr(self.inv[0]), ptr(self.inv[1]),
                                                ptr(maps), ptr(bmax), self.nb, int(normalize), ptr(S), st))
        torch.cuda.synchronize()

    def numpy_loop(self, normalize):
        """S, Q [n, F] float64: per sample the float32 map value (divided in float32 by the sample's
        band maximum when normalised), widened, added / squared and added."""
        S, Q = np.zeros((self.n, self.F)), np.zeros((self.n, self.F))
        valid = self.src >= 0
        for s in range(self.groups):
            v = self.maps[s * self.n:(s + 1) * self.n][:, self.src[valid]]
            if normalize:
                v = v / self.bmax[s, self.band[valid]][None, :]
            assert v.dtype == F32
            d = v.astype(F64)
            S[:, valid] = S[:, valid] + d
            Q[:, valid] = Q[:, valid] + d * d
        return S, Q


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("groups", [3, 11])
@pytest.mark.parametrize("name", list(PLANS_2D))
def test_frame_moments(P, name, groups, normalize):
    """wam_frame_moments_coef and wam_frame_moments: group_items 2, groups 3 (the scalar tail only) and 11
    (one block of 8 and a tail of 3). Both orders give equal bits; S is the frame
    wam_frame_accumulate_coef writes; S and Q are the numpy loop's bits; pixels outside the mosaic stay 0."""
    m = Frame2D(P, name, groups, 11 * groups + normalize)
    if name == "db4_J2_20x24":  # cropped bands: coefficients that reach no pixel, a non-square frame
        assert (host(m.inv[0]) < 0).any() and m.p.shape[0] != m.p.shape[1]
    out = {}
    for form in ("coef", "pixel"):
        S, Q = zeros64(m.n, m.F), zeros64(m.n, m.F)
        m.run(form, normalize, S, Q)
        out[form] = (host(S), host(Q))
    frame = zeros64(m.n, m.F)
    m.run("sum", normalize, frame, None)
    rS, rQ = m.numpy_loop(normalize)
    assert bits_equal(out["coef"][0], out["pixel"][0]) and bits_equal(out["coef"][1], out["pixel"][1])
    assert bits_equal(out["coef"][0], host(frame))
    assert bits_equal(out["coef"][0], rS)
    assert bits_equal(out["coef"][1], rQ)
    assert rQ.max() > 0 and not out["coef"][1][:, m.src < 0].any() and not out["coef"][0][:, m.src < 0].any()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("form", ["coef", "pixel"])
@pytest.mark.parametrize("name", list(PLANS_2D))
def test_frame_moments_chain(P, name, form, normalize):
    """Launches of 3 then 2 groups on the same accumulators give the bits of one launch of 5."""
    m = Frame2D(P, name, 5, 5)
    S1, Q1, S2, Q2 = (zeros64(m.n, m.F) for _ in range(4))
    m.run(form, normalize, S1, Q1)
    m.run(form, normalize, S2, Q2, 0, 3)
    m.run(form, normalize, S2, Q2, 3, 2)
    assert bits_equal(host(S1), host(S2)) and bits_equal(host(Q1), host(Q2))
    assert host(Q1).max() > 0


# ------------------------------------------------------------------------------ cube
CUBES = {"haar_8_J1": (8, 1, "strided"), "haar_8_J2": (8, 2, "strided"), "haar_6_J1": (6, 1, "consecutive")}


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", list(CUBES))
def test_cube_moments(P, name, offset):
    """wam_cube_moments, 2 items, 11 groups (two blocks of 4 samples' gathers and a tail of 3), signed
    map values: 8^3 x 2 = 1,024 voxels take the strided four-voxel form, 6^3 x 2 = 432 the consecutive
    one; offset 1: accumulator views one element (8 bytes) into their buffers, so the one-voxel
    (unaligned) form runs. S and Q are the numpy loop's bits, and launches of 3 then 8 give the same."""
    from wam_amd import frames
    size, J, form = CUBES[name]
    p = P.get_plan(3, (size,) * 3, J, "haar", "symmetric", "cuda")
    n, groups, L, K = 2, 11, size ** 3, p.coeff_numel
    src = frames.cube_map(p, size, torch.device("cuda", torch.cuda.current_device()))
    hs = host(src)
    assert (n * L % 256 == 0) == (form == "strided") and L % 4 == 0 and src.data_ptr() % 16 == 0
    maps = np.random.RandomState(size + J).standard_normal((groups * n, K)).astype(F32)

    def views():
        bufs = [torch.zeros(n * L + 2, dtype=torch.float64, device="cuda") for _ in range(2)]
        v = [b[offset:offset + n * L] for b in bufs]
        assert all(t.data_ptr() % 16 == 8 * offset for t in v)
        return v, bufs

    (S, Q), keep = views()
    P.cube_moments(groups, n, src, dev(maps), K, S, Q)
    (S2, Q2), keep2 = views()
    P.cube_moments(3, n, src, dev(maps[:3 * n]), K, S2, Q2)
    P.cube_moments(8, n, src, dev(maps[3 * n:]), K, S2, Q2)
    torch.cuda.synchronize()
    rS, rQ = np.zeros((n, L)), np.zeros((n, L))
    for s in range(groups):
        d = np.where(hs >= 0, maps[s * n:(s + 1) * n][:, np.maximum(hs, 0)], F32(0)).astype(F64)
        rS, rQ = rS + d, rQ + d * d
    assert bits_equal(host(S).reshape(n, L), rS) and bits_equal(host(Q).reshape(n, L), rQ)
    assert bits_equal(host(S), host(S2)) and bits_equal(host(Q), host(Q2))
    for b in keep + keep2:  # nothing written beside the views
        hb = host(b)
        assert not hb[:offset].any() and not hb[offset + n * L:].any()


# ------------------------------------------------------------------------------ 1D stream
@pytest.mark.parametrize("length", [1000, 1003])
def test_moments_f32(P, length):
    """wam_moments_f32, 11 groups, lengths 1,000 and 1,003 (several blocks, the last one partial)."""
    groups = 11
    src = np.random.RandomState(length).standard_normal((groups, length)).astype(F32)
    S, Q, S2, Q2 = (zeros64(length) for _ in range(4))
    P.moments_f32(dev(src), groups, S, Q)
    P.moments_f32(dev(src[:3]), 3, S2, Q2)
    P.moments_f32(dev(src[3:]), 8, S2, Q2)
    rS, rQ = np.zeros(length), np.zeros(length)
    for s in range(groups):
        d = src[s].astype(F64)
        rS, rQ = rS + d, rQ + d * d
    assert bits_equal(host(S), rS) and bits_equal(host(Q), rQ)
    assert bits_equal(host(S), host(S2)) and bits_equal(host(Q), host(Q2))


# ------------------------------------------------------------------------------ finish
def _sq(n, length, seed):
    v = np.random.RandomState(seed).uniform(-1, 1, (n, length)).astype(F32).astype(F64)
    S, Q = np.zeros(length), np.zeros(length)
    for s in range(n):
        S, Q = S + v[s], Q + v[s] * v[s]
    return S, Q


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_moments_finish(P, dtype):
    """wam_moments_finish on 1,003 elements, n = 6: the quotients S / n and Q / n are numpy's bits (as
    float64, or that value rounded once to float32); the variance is within 2^-49 max(Q / n) of numpy's
    max(Q / n - m m, 0) -- four roundings (S / n, Q / n, numpy's m m and its subtraction against the one
    fused step), each at most half an ulp of a quantity no larger than Q / n since m^2 <= Q / n -- plus,
    for a float32 output, its own rounding."""
    n, L = 6, 1003
    S, Q = _sq(n, L, 1)
    np_dt = F64 if dtype == torch.float64 else F32
    got = {k: host(P.moments_finish(dev(S), dev(Q), n, k, dtype)) for k in P.MOMENT_KINDS}
    assert bits_equal(got["mean"], (S / n).astype(np_dt))
    assert bits_equal(got["smooth_sq"], (Q / n).astype(np_dt))
    m = S / n
    ref = np.maximum(Q / n - m * m, 0.0)
    bound = 2.0 ** -49 * (Q / n).max()
    if dtype == torch.float32:
        bound = bound + 2.0 ** -24 * ref
    err = np.abs(got["vargrad"].astype(F64) - ref)
    print("[moments] finish vargrad %s: max err %.3e, bound %.3e, max ref %.3e" % (np_dt.__name__, err.max(),
                                                                                   np.max(bound), ref.max()))
    assert (err <= bound).all() and (got["vargrad"] >= 0).all() and ref.max() > 0.1


def test_moments_finish_n1_and_nan(P):
    """n = 1: S = v, Q = v v exactly, so the variance is all-zero bits. A NaN map value (through
    wam_moments_f32) gives NaN in all three kinds at that element and nowhere else."""
    v = np.random.RandomState(2).uniform(-3, 3, (1, 1003)).astype(F32)
    S, Q = zeros64(1003), zeros64(1003)
    P.moments_f32(dev(v), 1, S, Q)
    for dt in (torch.float64, torch.float32):
        out = host(P.moments_finish(S, Q, 1, "vargrad", dt))
        assert not out.view(np.uint8).any()
    assert bits_equal(host(P.moments_finish(S, Q, 1, "mean")), v[0].astype(F64))
    w = np.random.RandomState(3).uniform(0, 1, (3, 1003)).astype(F32)
    w[1, 700] = np.nan
    S, Q = zeros64(1003), zeros64(1003)
    P.moments_f32(dev(w), 3, S, Q)
    for kind in P.MOMENT_KINDS:
        for dt in (torch.float64, torch.float32):
            out = host(P.moments_finish(S, Q, 3, kind, dt))
            assert np.array_equal(np.isnan(out), np.arange(1003) == 700), kind


# ------------------------------------------------------------------------------ refusals
def test_argument_errors_launch_nothing(P):
    """The host checks of the five entries on 2 items, a frame of 5 pixels, 7 coefficients, 2 bands, 2
    groups: every required pointer NULL in turn, every checked count negative, normalize without
    band_max, a finish with n = 0, kind 3 / -1, both or neither output, or without the accumulator its
    kind reads all return WAM_ERR_INVALID_ARG; zero groups and zero work return WAM_OK; and no output
    buffer (filled with 7) changes a bit. Valid arguments would change them: the maps are all ones."""
    from wam_amd._lib import lib, ptr, stream_of
    n, F, K, nb, G = 2, 5, 7, 2, 2
    i32 = lambda *v: dev(np.array(v, np.int32))
    src, band = i32(3, -1, 0, 6, 2), i32(1, 0, 0, 1, 0)
    dst, cband = i32(2, -1, 4, 0, -1, -1, 3), i32(0, 0, 0, 1, 1, 1, 1)
    ones = lambda *shape: torch.ones(shape, device="cuda")
    maps, bmax, stream = ones(G * n, K), ones(G, nb), ones(G, n * F)
    outs = {k: torch.full((n * F,), 7.0, dtype=dt, device="cuda")
            for k, dt in (("S", torch.float64), ("Q", torch.float64), ("o64", torch.float64), ("o32", torch.float32))}
    st = stream_of(maps.device)

    def entry(fn, order, **defaults):
        def call(**kw):
            a = dict(defaults, **kw)
            return fn(*[a[k] if isinstance(a[k], (int, float)) else ptr(a[k]) for k in order.split()], st)
        return call

    base = dict(groups=G, n=n, F=F, K=K, src=src, band=band, dst=dst, cband=cband, maps=maps, bmax=bmax, nb=nb, norm=1,
                len=n * F, stream=stream, N=6, kind=2, none=None, **outs)
    table = [
        (entry(lib.wam_frame_moments, "groups n F src band maps K bmax nb norm S Q", **base),
         "src band maps S Q", "groups n F", [{"bmax": None}], [{"groups": 0}, {"n": 0}, {"F": 0}]),
        (entry(lib.wam_frame_moments_coef, "groups n K F dst cband maps bmax nb norm S Q", **base),
         "dst cband maps S Q", "groups n K F", [{"bmax": None}], [{"groups": 0}, {"n": 0}, {"K": 0}]),
        (entry(lib.wam_cube_moments, "groups n F src maps K S Q", **base),
         "src maps S Q", "groups n F K", [], [{"groups": 0}, {"n": 0}, {"F": 0}]),
        (entry(lib.wam_moments_f32, "groups len stream S Q", **base),
         "stream S Q", "groups len", [], [{"groups": 0}, {"len": 0}]),
        (entry(lib.wam_moments_finish, "len S Q N kind o64 none", **base),
         "o64", "len", [{"N": 0}, {"N": -1}, {"kind": 3}, {"kind": -1}, {"none": outs["o32"]}, {"S": None},
                        {"Q": None}, {"kind": 0, "S": None}, {"kind": 1, "Q": None}], [{"len": 0}]),
    ]
    for call, pointers, counts, refused, nothing in table:
        for kw in [{k: None} for k in pointers.split()] + [{k: -1} for k in counts.split()] + refused:
            assert call(**kw) == INVALID, kw
        for kw in nothing:
            assert call(**kw) == OK, kw
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == 7.0).all()), k


# ------------------------------------------------------------------------------ classes
@pytest.fixture(scope="module")
def W():
    import wam_amd
    return wam_amd


def _ex2d(W, name, method, **kw):
    c = M.CASES_2D[name]
    return W.WaveletAttribution2D(testmodels.TinySmooth2D().cuda(), wavelet=c["wavelet"], J=c["J"], method=method,
                                  n_samples=M.N_SAMPLES, stdev_spread=M.SPREAD_2D, random_seed=M.SEED, frame="native",
                                  **kw)


@pytest.mark.parametrize("name", list(M.CASES_2D))
def test_wam2d_moments(W, name):
    """WaveletAttribution2D 'smooth_sq' / 'vargrad' on the two CPU-checked inputs (TinySmooth2D, numpy
    noise, 6 samples, native frame): float64 [N, H, W]; smooth_mean bit-identical to a 'smooth' run of the
    same seed; smooth_sq within 2e-4 and vargrad within 4e-4 (max abs) of tests/moments_ref.py -- under
    1 % of the reference maxima (>= 0.04, tests/test_moments_ref.py); .scales is the reprojection of the
    returned map."""
    ref = M.ref_2d(name)
    x = M.inputs_2d(name)
    smooth = _ex2d(W, name, "smooth")(x, M.LABELS_2D)
    for method, bar in (("smooth_sq", 2e-4), ("vargrad", 4e-4)):
        ex = _ex2d(W, name, method)
        out = ex(x, M.LABELS_2D)
        assert out.dtype == F64 and out.shape == ref[method].shape == smooth.shape
        assert bits_equal(ex.smooth_mean, smooth)
        err = float(np.abs(out - ref[method]).max())
        print("[moments] 2D %s %s: max err %.3e (bar %.0e), reference max %.4f" % (name, method, err, bar,
                                                                                  ref[method].max()))
        assert err < bar
        assert bar < 0.01 * ref["vargrad"].max()
        assert ex.scales.shape == (2, M.CASES_2D[name]["J"], x.shape[-1], x.shape[-1])
        assert bits_equal(ex.scales, ex.reproject_wam(out, ex.J))
        assert bits_equal(host(ex.map_device), out)


@pytest.mark.parametrize("noise", ["numpy", "philox"])
def test_wam2d_sample_batch_gives_equal_bits(W, noise):
    """sample_batch=1 (six model calls, six accumulator launches of one group) against the default (one
    call of six samples, one launch): equal bits of the variance and of smooth_mean, on both noise modes."""
    x = M.inputs_2d("haar_J2_32")
    a = _ex2d(W, "haar_J2_32", "vargrad", noise=noise)
    b = _ex2d(W, "haar_J2_32", "vargrad", noise=noise, sample_batch=1)
    oa, ob = a(x, M.LABELS_2D), b(x, M.LABELS_2D)
    print("[moments] sample_batch: max |d vargrad| %.3e, max |d mean| %.3e" % (
        np.abs(oa - ob).max(), np.abs(a.smooth_mean - b.smooth_mean).max()))
    assert oa.max() > 0
    assert bits_equal(oa, ob) and bits_equal(a.smooth_mean, b.smooth_mean)


def _rel_to(got, ref, scale):
    return float(np.abs(np.asarray(got, dtype=F64) - ref).max() / scale)


def test_wam1d_moments(W):
    """WaveletAttribution1D (TinyAudio, db6 J=2, 4,096 samples, numpy noise, 6 samples): (mel, [bands])
    float32 of 'smooth''s shapes; per array, smooth_sq within 2e-4 and vargrad within 4e-4 of max(Q / n)
    of the restatement; smooth_mean within the suite's 1e-4 of the maximum; melspecs / grad_coeffs set."""
    ref = M.ref_1d()
    x = M.inputs_1d()
    kw = dict(M.KW_1D, n_samples=M.N_SAMPLES, random_seed=M.SEED)
    for method, bar in (("smooth_sq", 2e-4), ("vargrad", 4e-4)):
        ex = W.WaveletAttribution1D(testmodels.TinyAudio().cuda(), method=method, **kw)
        mel, cs = ex(x, M.LABELS_1D)
        assert ex.melspecs is mel and ex.grad_coeffs is cs and len(cs) == 3
        got = [mel] + list(cs)
        want = [ref[method][0]] + list(ref[method][1])
        qn = [ref["smooth_sq"][0]] + list(ref["smooth_sq"][1])
        mean = [ref["mean"][0]] + list(ref["mean"][1])
        sm = [ex.smooth_mean[0]] + list(ex.smooth_mean[1])
        for j, (g, r, q, mr, mg) in enumerate(zip(got, want, qn, mean, sm)):
            assert g.dtype == F32 and g.shape == r.shape and mg.shape == mr.shape
            err = _rel_to(g, r, q.max())
            print("[moments] 1D %s part %d: err / max(Q/n) %.3e (bar %.0e), max(Q/n) %.4e, reference max %.4e"
                  % (method, j, err, bar, q.max(), r.max()))
            assert err < bar and r.max() > 0
            assert _rel_to(mg, mr, np.abs(mr).max()) < 1e-4


def test_wam3d_moments(W):
    """WaveletAttribution3D (TinyVoxel, Haar J=2 at 16^3, stdev_spread 0.05, numpy noise, 6 samples): a
    float32 cube; smooth_sq within 2e-4 and vargrad within 4e-4 of max(Q / n); smooth_mean is the PLAIN
    mean (1e-4 of its maximum), not the legacy in-loop average 'smooth' returns; .grads set."""
    ref = M.ref_3d()
    x = M.inputs_3d()
    kw = dict(M.KW_3D, n_samples=M.N_SAMPLES, random_seed=M.SEED)
    qmax = ref["smooth_sq"].max()
    for method, bar in (("smooth_sq", 2e-4), ("vargrad", 4e-4)):
        ex = W.WaveletAttribution3D(testmodels.TinyVoxel().cuda(), method=method, **kw)
        out = ex(x, M.LABELS_3D)
        assert out.dtype == F32 and out.shape == ref[method].shape and ex.grads is out
        err = _rel_to(out, ref[method], qmax)
        print("[moments] 3D %s: err / max(Q/n) %.3e (bar %.0e), max(Q/n) %.4e, reference max %.4e"
              % (method, err, bar, qmax, ref[method].max()))
        assert err < bar and ref[method].max() > 0
        assert _rel_to(ex.smooth_mean, ref["mean"], ref["mean"].max()) < 1e-4
    legacy = W.WaveletAttribution3D(testmodels.TinyVoxel().cuda(), method="smooth", **kw)(x, M.LABELS_3D)
    assert _rel_to(legacy, ref["mean"], ref["mean"].max()) > 0.1


def test_eval3d_forwards_vargrad(W):
    """Eval3DWAM(method='vargrad').insertion at 8^3, J=1, n_iter=4: the inner explainer gets the method,
    is called once, and the scores are finite."""
    from wam_amd.evaluation import Eval3DWAM
    ev = Eval3DWAM(testmodels.TinyVoxel().cuda(), wavelet="haar", J=1, method="vargrad", n_samples=3,
                   stdev_spread=0.05)
    calls = []
    inner = ev.gradwam
    ev.gradwam = lambda *a: calls.append(1) or inner(*a)
    x = torch.rand(2, 1, 8, 8, 8, generator=torch.Generator().manual_seed(8))
    scores = ev.insertion(x, [1, 2], n_iter=4)
    scores2 = ev.insertion(x, [1, 2], n_iter=4)
    assert inner.method == "vargrad" and len(calls) == 1
    assert len(scores) == 2 and np.isfinite(scores).all() and scores == scores2
    assert ev.grad_wams.shape == (2, 8, 8, 8) and ev.grad_wams.max() > 0 and inner.smooth_mean is not None


def test_unknown_method_still_falls_through(W):
    """The fall-through of unknown method names is unchanged: None, no error."""
    ex = W.WaveletAttribution2D(testmodels.TinySmooth2D().cuda(), wavelet="haar", J=2, method="nope", n_samples=2,
                                frame="native")
    assert ex(M.inputs_2d("haar_J2_32"), M.LABELS_2D) is None
