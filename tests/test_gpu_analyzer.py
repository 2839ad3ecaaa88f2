"""WAMAnalyzer2D on the device: the entries of wam_amd/csrc/analyze2d.hip at the C ABI, bit for bit
against the numpy references of tests/analyzer_ref.py; the module functions against the goldens made
by the reference's own helpers (tests/golden/analyzer_goldens.npz); the class end to end against the
restatement run with the same model on the CPU.

Bars: thresholds and masks exact. Float images within 4 * R.D32 of the golden relative to its
maximum (R.float_distance): D32 = 4.8e-7 is what the float64 restatement leaves against float32 pywt
on the CPU (tests/test_analyzer_ref.py), the factor 4 is the 1-D evaluator's, for a device that sums
each Haar level in another order than pywt. uint8 images: circular grey-level distance <= 1, share of
pixels at non-zero distance <= R.CAP = 1e-3 (tests/test_gpu_eval.py's cap). Probabilities within 1e-4
(the 2D evaluator's bar); the end-to-end case's top two logits are 0.075 apart or more (750 bars,
asserted on the CPU side of the test).

Measured on one MI355X (printed when the module finishes): worst float distance 5.36e-7 (bar 1.9e-6), worst
uint8 share 8.1e-5 (cap 1e-3), worst |dp| 1.8e-6 (bar 1e-4).
"""
import ctypes

import numpy as np
import pytest
import torch

import testmodels
from tests import analyzer_ref as R
from tests.golden import analyzer_cases as C
from tests.helpers import npz

pytestmark = pytest.mark.gpu
WORST = {"float": 0.0, "share": 0.0, "dp": 0.0}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()
    print("[analyzer] worst float distance %.3e (bar %.1e), worst uint8 share %.2e (cap %.0e), worst |dp| %.3e"
          % (WORST["float"], 4 * R.D32, WORST["share"], R.CAP, WORST["dp"]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(packed, shape):
    return np.unpackbits(packed)[:int(np.prod(shape))].reshape(shape).astype(bool)


# ------------------------------------------------------------------------------ wam_threshold_mask_coeffs
def run_threshold(L, plan, N, Cn, size, wam, thr, n_thr, stride, level=0, edges=None, strict=0, pos=None, seed=0):
    """One call against threshold_mask_coeffs_ref on random coefficients: bit-equal."""
    from wam_amd.evaluation import coeff_array_layout
    off = list(plan.band_offsets)
    K = off[-1]
    if pos is None:
        pos, shape = coeff_array_layout(plan)
        assert shape == (size, size)
    pos = np.asarray(pos, dtype=np.int32)
    coeffs = np.random.RandomState(seed).standard_normal(N * Cn * K).astype(np.float32)
    dc, dp, dw, dt = dev(coeffs), dev(pos), dev(wam.reshape(N, -1)), dev(thr.reshape(-1))
    out = torch.full((N * n_thr * Cn * K,), 7.0, device="cuda")
    assert dc.data_ptr() % 16 == 0 and dp.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    ed = None if edges is None else (ctypes.c_int32 * len(edges))(*edges)
    L.check(L.lib.wam_threshold_mask_coeffs(plan.handle, N, Cn, L.ptr(dc), L.ptr(dp), size, L.ptr(dw), n_thr, L.ptr(dt),
                                            stride, level, ed, strict, L.ptr(out), L.stream_of(out.device)))
    ref = R.threshold_mask_coeffs_ref(off, N, Cn, coeffs, pos, size, wam, n_thr, thr, stride, level, edges, strict)
    R.assert_bits(out.cpu().numpy(), ref, "threshold_mask level=%d strict=%d" % (level, strict))
    return out, dc, ref, coeffs


def quantile_rows(wams, qs, stride=None):
    stride = len(qs) if stride is None else stride
    thr = np.full((len(wams), stride), np.nan)   # the padding of a wider row is never read
    for n, w in enumerate(wams):
        thr[n, :len(qs)] = [R.quantile(w, q) for q in qs]
    return thr


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("name", ["haar_32_J2", "haar_64_J3", "channels_1", "stride_8"])
def test_threshold_mask_quantiles(L, name, strict):
    """Quantile thresholds (q = 0 and q = 1 among them: the threshold equals an element of the map, so
    the two `strict` values select different sets) on Haar plans, whose bands are all multiples of 4
    (the 16-byte path): 3 images x 5 thresholds x 3 channels at 32^2; 64^2 J=3; one channel; rows of 8
    thresholds of which 5 are used."""
    from wam_amd.plan import get_plan
    size, J, N, Cn, stride = {"haar_32_J2": (32, 2, 3, 3, 5), "haar_64_J3": (64, 3, 2, 3, 5),
                              "channels_1": (32, 2, 3, 1, 5), "stride_8": (32, 2, 2, 3, 8)}[name]
    plan = get_plan(2, (size, size), J, "haar", "symmetric", "cuda")
    assert all(o % 4 == 0 for o in plan.band_offsets)
    wams = np.stack([C.make_map(size, 100 * size + n) for n in range(N)])
    thr = quantile_rows(wams, C.QS, stride)
    out, dc, ref, coeffs = run_threshold(L, plan, N, Cn, size, wams, thr, 5, stride, strict=strict, seed=size + strict)
    K = plan.coeff_numel
    if not strict:   # q = 0 keeps everything: wam_waverec of those planes is the unmasked reconstruction
        rec = plan.waverec(out, N * 5 * Cn)[0].view(N, 5, Cn, size, size)
        assert torch.equal(rec[:, 0], plan.waverec(dc, N * Cn)[0].view(N, Cn, size, size))
    else:            # strict at q = 1 drops everything
        off = plan.band_offsets
        for o0, o1 in zip(off[:-1], off[1:]):
            assert not ref[N * 5 * Cn * o0:N * 5 * Cn * o1].reshape(N, 5, Cn, o1 - o0)[:, 4].any()
        assert K > 0


@pytest.mark.parametrize("strict", [0, 1])
def test_threshold_mask_ties(L, strict):
    """A map of 16 distinct values (64 ties each) whose thresholds are map values: >= and > differ by
    whole tie groups, bit-equal under both."""
    from wam_amd.plan import get_plan
    plan = get_plan(2, (32, 32), 2, "haar", "symmetric", "cuda")
    rs = np.random.RandomState(77)
    wams = rs.randint(0, 16, (2, 32, 32)).astype(np.float64) / 8.0
    thr = np.array([[0.0, 0.5, 1.0, 1.875], [0.125, 0.75, 1.5, 2.0]])
    _, _, ref, coeffs = run_threshold(L, plan, 2, 3, 32, wams, thr, 4, 4, strict=strict, seed=5)
    other = R.threshold_mask_coeffs_ref(list(plan.band_offsets), 2, 3, coeffs, plan_pos(plan), 32, wams, 4, thr, 4, 0,
                                        None, 1 - strict)
    assert not np.array_equal(ref, other)


def plan_pos(plan):
    from wam_amd.evaluation import coeff_array_layout
    return coeff_array_layout(plan)[0].astype(np.int32)


@pytest.mark.parametrize("size,J", [(32, 2), (64, 3)])
def test_threshold_mask_level_mode(L, size, J):
    """Level mode with J + 1 entries: thresholds min(0, region min) + EPS, strict, edges int(S / 2^j).
    One map is strictly positive, one has negative values in some regions (the minimum then comes from
    the region, not from the zeros around it)."""
    from wam_amd.plan import get_plan
    plan = get_plan(2, (size, size), J, "haar", "symmetric", "cuda")
    wams = np.stack([C.make_map(size, 9), C.make_map(size, 10) - 0.8])
    thr = np.stack([[R.levelized_masks(w, J)[l].min() + C.EPS for l in range(J + 1)] for w in wams])
    assert (thr[0] == C.EPS).all() and (thr[1] < 0).any()
    run_threshold(L, plan, 2, 3, size, wams, thr, J + 1, J + 1, level=1, edges=R.level_edges(size, J), strict=1, seed=J)


def test_threshold_mask_db2_scalar_and_vector_paths(L):
    """db2 at 32^2, J=2: pywt's array is 37 x 37, the bands hold 100, 100, 100, 100, 289, 289, 289
    values at offsets 0 .. 400, 689, 978: the first five bands start on a multiple of 4 and the first
    four take the 16-byte path, the rest the scalar one. Plus one position outside the array and one
    negative: kept by no threshold. The kernel does not care that the class refuses db2."""
    from wam_amd.plan import get_plan
    plan = get_plan(2, (32, 32), 2, "db2", "symmetric", "cuda")
    assert np.diff(plan.band_offsets).tolist() == [100, 100, 100, 100, 289, 289, 289]
    pos = plan_pos(plan).copy()
    pos[7], pos[500] = 37 * 37 + 3, -1
    wams = np.stack([C.make_map(37, n) for n in range(3)])
    thr = quantile_rows(wams, C.QS)
    for strict in (0, 1):
        run_threshold(L, plan, 3, 3, 37, wams, thr, 5, 5, strict=strict, pos=pos, seed=37)


def test_threshold_mask_more_thresholds_than_one_chunk(L):
    """40 thresholds: three blockIdx.y chunks of 16, the last one partial."""
    from wam_amd.plan import get_plan
    plan = get_plan(2, (32, 32), 2, "haar", "symmetric", "cuda")
    wams = np.stack([C.make_map(32, 1)])
    qs = np.linspace(0, 1, 40)
    run_threshold(L, plan, 1, 3, 32, wams, quantile_rows(wams, qs), 40, 40, seed=40)


def test_threshold_mask_rejected_calls(L):
    from wam_amd.plan import get_plan
    p2 = get_plan(2, (32, 32), 2, "haar", "symmetric", "cuda")
    p1 = get_plan(1, (64,), 2, "haar", "reflect", "cuda")
    p3 = get_plan(3, (8, 8, 8), 1, "haar", "reflect", "cuda")
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    call = lambda p, images, n_thr: L.lib.wam_threshold_mask_coeffs(  # noqa: E731
        p.handle, images, 1, L.ptr(buf), L.ptr(buf), 32, L.ptr(buf), n_thr, L.ptr(buf), max(n_thr, 1), 0, None, 0,
        L.ptr(buf), L.stream_of(buf.device))
    assert call(p1, 1, 1) == 3 and call(p3, 1, 1) == 3      # WAM_ERR_UNSUPPORTED
    assert call(p2, 1, 0) == 1 and call(p2, 0, 1) == 1      # WAM_ERR_INVALID_ARG


# ------------------------------------------------------------------------------ quantisation
def quant_inputs(plane=1000):
    """5 images x 3 channels x `plane` values (1000: the 16-byte path; 999: the scalar one). [0] is
    positive (mn > 0: s falls below 0); [1] has a small
    positive maximum and a negative minimum (s runs past 255 and past 511); [2] a constant zero image
    (0 / 0 -> NaN -> 0); [3] a constant non-zero image; [4] a maximum of 0 (division by zero: +-inf and
    NaN -> 0)."""
    rs = np.random.RandomState(3)
    rec = np.empty((5, 3, plane), dtype=np.float32)
    rec[0] = rs.uniform(0.2, 1.0, (3, plane))
    rec[1] = rs.uniform(-0.5, 0.25, (3, plane))
    rec[2] = 0.0
    rec[3] = 0.37
    rec[4] = -np.abs(rs.uniform(0.1, 1.0, (3, plane)))
    rec[4, 1, 5] = 0.0
    return rec


@pytest.mark.parametrize("plane", [1000, 999])
def test_quantize_rule1_bit_equal(L, plane):
    from wam_amd.evaluation import IMAGENET_MEAN, IMAGENET_STD
    rec = quant_inputs(plane)
    s = [((x - x.min()) / x.max() - x.min()) * np.float32(255) for x in rec[:2]]
    assert (s[0] < 0).any() and (s[1] > 255).any() and (s[1] > 511).any()   # the premise: all three wrap ranges occur
    mean, std = (L.c_f32 * 3)(*IMAGENET_MEAN), (L.c_f32 * 3)(*IMAGENET_STD)
    d = dev(rec)
    n = rec.shape[0]
    u8 = torch.full(rec.shape, 9, dtype=torch.uint8, device="cuda")
    out = torch.full(rec.shape, 7.0, device="cuda")
    L.check(L.lib.wam_quantize_normalize_ex(n, 3, plane, L.ptr(d), 1, mean, std, L.ptr(u8), L.ptr(out),
                                            L.stream_of(d.device)))
    ref_u8, ref_out = R.quantize_ref(rec, 1, IMAGENET_MEAN, IMAGENET_STD)
    assert np.array_equal(u8.cpu().numpy(), ref_u8)
    R.assert_bits(out.cpu().numpy(), ref_out, "quantize rule 1")
    assert (ref_u8[2] == 0).all() and (ref_u8[4] == 0).all()
    # either output alone gives the same values
    u8b = torch.empty_like(u8)
    outb = torch.empty_like(out)
    L.check(L.lib.wam_quantize_normalize_ex(n, 3, plane, L.ptr(d), 1, None, None, L.ptr(u8b), None, L.stream_of(d.device)))
    L.check(L.lib.wam_quantize_normalize_ex(n, 3, plane, L.ptr(d), 1, mean, std, None, L.ptr(outb), L.stream_of(d.device)))
    assert torch.equal(u8b, u8) and torch.equal(outb.view(torch.int32), out.view(torch.int32))
    assert L.lib.wam_quantize_normalize_ex(n, 3, plane, L.ptr(d), 1, mean, std, None, None, L.stream_of(d.device)) == 1
    assert L.lib.wam_quantize_normalize_ex(n, 3, plane, L.ptr(d), 2, mean, std, L.ptr(u8), None, L.stream_of(d.device)) == 1


@pytest.mark.parametrize("plane", [1000, 999])
def test_quantize_rule0_equals_the_old_entry(L, plane):
    from wam_amd.evaluation import IMAGENET_MEAN, IMAGENET_STD
    rec = quant_inputs(plane)
    mean, std = (L.c_f32 * 3)(*IMAGENET_MEAN), (L.c_f32 * 3)(*IMAGENET_STD)
    d = dev(rec)
    old, new = torch.empty_like(d), torch.empty_like(d)
    u8 = torch.empty(rec.shape, dtype=torch.uint8, device="cuda")
    L.check(L.lib.wam_quantize_normalize(5, 3, plane, L.ptr(d), mean, std, L.ptr(old), L.stream_of(d.device)))
    L.check(L.lib.wam_quantize_normalize_ex(5, 3, plane, L.ptr(d), 0, mean, std, L.ptr(u8), L.ptr(new),
                                            L.stream_of(d.device)))
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))
    ref_u8, ref_out = R.quantize_ref(rec, 0, IMAGENET_MEAN, IMAGENET_STD)
    assert np.array_equal(u8.cpu().numpy(), ref_u8)
    R.assert_bits(new.cpu().numpy(), ref_out, "quantize rule 0")


@pytest.mark.parametrize("size", [64, 32])
@pytest.mark.parametrize("rule", [1, 0])
def test_resize_path_equals_pillow(L, size, rule):
    """wam_quantize_resize_normalize_ex at size^2 -> 224^2: PIL.Image.resize of the emulated bytes, then
    ToTensor + Normalize, exactly; rule 0 also equals the old entry point."""
    from wam_amd.evaluation import IMAGENET_MEAN, IMAGENET_STD, resize_default
    rs = np.random.RandomState(size + rule)
    rec = rs.uniform(-0.3, 1.1, (3, 3, size * size)).astype(np.float32)
    rec[1] = 0.0
    mean, std = (L.c_f32 * 3)(*IMAGENET_MEAN), (L.c_f32 * 3)(*IMAGENET_STD)
    d = dev(rec)
    got, u8 = resize_default(d.device, d, 3, 3, size, size, mean, std, rule=rule)
    ref_u8, _ = R.quantize_ref(rec, rule)
    assert np.array_equal(u8.cpu().numpy(), ref_u8)
    for i in range(3):
        hwc = np.ascontiguousarray(np.moveaxis(ref_u8[i].reshape(3, size, size), 0, 2))
        assert torch.equal(got[i].cpu(), R.to_input(hwc)), i
    if rule == 0:
        ev_out = wam_eval(L)._resize_default(d, 3, 3, size, size, mean, std)
        assert torch.equal(ev_out, got)


def wam_eval(L):
    import wam_amd
    return wam_amd.Eval2DWAM(testmodels.TinySmooth2D().cuda(), wavelet="haar", J=3)


# ------------------------------------------------------------------------------ module functions vs goldens
def test_thresholds_on_the_device_are_numpy_quantiles(L):
    from wam_amd.analysis import level_thresholds, quantile_thresholds
    g = npz(C.GOLDENS)
    for name, (size, J, seed, chans, qs) in list(C.PARTIAL.items()) + list(C.QUIRK.items()):
        wam = C.make_map(size, seed)
        thr = quantile_thresholds(dev(wam.reshape(1, -1)), qs).cpu().numpy()[0]
        assert np.array_equal(thr, g[C.key("thr", name)]), name
    wam = C.make_map(32, 3201)
    sweep = np.random.RandomState(11).uniform(size=500)
    assert np.array_equal(quantile_thresholds(dev(wam.reshape(1, -1)), sweep).cpu().numpy()[0], np.quantile(wam, sweep))
    wams = np.stack([C.make_map(32, 9), C.make_map(32, 10) - 0.8])
    lt = level_thresholds(dev(wams.reshape(2, -1)), 32, 2, C.EPS).cpu().numpy()
    want = np.stack([[R.levelized_masks(w, 2)[l].min() + C.EPS for l in range(3)] for w in wams])
    assert np.array_equal(lt, want)


@pytest.mark.parametrize("name", list(C.PARTIAL))
def test_generate_partial_image_vs_goldens(L, name):
    from wam_amd.analysis import generate_partial_image
    g = npz(C.GOLDENS)
    size, J, seed, chans, qs = C.PARTIAL[name]
    img, wam = C.make_image(size, seed), C.make_map(size, seed)
    for q in qs:
        image, mask = generate_partial_image(img, wam, q, J, wavelet="haar")
        assert image.dtype == np.float32 and image.shape == (size, size, 3)
        assert np.array_equal(mask, bits(g[C.key("pmask", name, q)], (size, size)) * wam), q
        d = R.float_distance(image[:, :, list(chans)], g[C.key("partial", name, q)])
        print("[analyzer] partial %s q=%.2f: d = %.3e" % (name, q, d))
        WORST["float"] = max(WORST["float"], d)
        assert d <= 4 * R.D32, (name, q, d)


@pytest.mark.parametrize("name", list(C.LEVELS))
def test_generate_disentangled_images_vs_goldens(L, name):
    from wam_amd.analysis import compute_levelized_masks, generate_disentangled_images
    g = npz(C.GOLDENS)
    size, J, seed, chans = C.LEVELS[name]
    img, wam = C.make_image(size, seed), C.make_map(size, seed)
    images, filtered = generate_disentangled_images(wam, img, J, EPS=C.EPS, wavelet="haar")
    assert images.dtype == np.float64 and images.shape == (J + 1, size, size, 3)
    assert filtered.dtype == np.float64
    assert np.array_equal(filtered, bits(g[C.key("lmask", name)], (J + 1, size, size)) * wam[None])
    assert np.array_equal(filtered, compute_levelized_masks(wam, J))
    d = R.float_distance(images[..., list(chans)], g[C.key("levels", name)])
    print("[analyzer] levels %s: d = %.3e" % (name, d))
    WORST["float"] = max(WORST["float"], d)
    assert d <= 4 * R.D32, (name, d)
    assert images.min() >= 0


@pytest.mark.parametrize("name", list(C.QUIRK))
def test_quirk_quantised_images_vs_goldens(L, name):
    """The bytes the class hands to PIL (normalize='reference') against the reference's own uint8 image."""
    import wam_amd
    g = npz(C.GOLDENS)
    size, J, seed, chans, qs = C.QUIRK[name]
    img, wam = C.make_image(size, seed), C.make_map(size, seed)
    an = wam_amd.WAMAnalyzer2D(testmodels.TinySmooth2D().cuda(), wavelet="haar", J=J)
    an.grad_wams = wam[None]
    seen = []
    x = torch.tensor(np.moveaxis(img, 2, 0)[None])
    an.isolate_necessary_components(x, [0], list(qs), transform=lambda im: seen.append(np.asarray(im)) or
                                    torch.zeros(3, 224, 224), mode="deletion")   # ascending quantiles
    assert len(seen) == len(qs)
    for q, u8 in zip(qs, seen):
        mx, share = R.u8_compare(np.ascontiguousarray(u8[:, :, list(chans)]), g[C.key("quirk", name, q)])
        print("[analyzer] quirk %s q=%.2f: max circular distance %d, share %.2e" % (name, q, mx, share))
        WORST["share"] = max(WORST["share"], share)
        assert mx <= 1 and share <= R.CAP, (name, q, mx, share)


# ------------------------------------------------------------------------------ the class end to end
def make_analyzer(**kw):
    import wam_amd
    x, gw = C.make_e2e()
    an = wam_amd.WAMAnalyzer2D(testmodels.TinySmooth2D(seed=C.E2E_MODEL_SEED).cuda(), wavelet="haar", J=C.E2E_J, **kw)
    an.grad_wams = gw
    return an, torch.tensor(x), gw


@pytest.fixture(scope="module")
def e2e_ref():
    """The restatement with the same model on the CPU, both modes, computed once."""
    x, gw = C.make_e2e()
    model = testmodels.TinySmooth2D(seed=C.E2E_MODEL_SEED)
    out = {}
    for mode, qs in (("insertion", list(C.E2E_QS)), ("deletion", list(C.E2E_QS)[::-1])):
        out[mode] = R.isolate_necessary_components(model, torch.tensor(x), list(C.E2E_LABELS), gw, qs, mode, C.E2E_J)
    return out


@pytest.mark.parametrize("mode", ["insertion", "deletion"])
def test_end_to_end_vs_restatement(L, e2e_ref, mode):
    from PIL import Image
    qs = list(C.E2E_QS) if mode == "insertion" else list(C.E2E_QS)[::-1]
    an, x, gw = make_analyzer()
    outs = an.isolate_necessary_components(x, list(C.E2E_LABELS), qs, mode=mode)
    ref_outs, ref_q = e2e_ref[mode]
    got_q = an.insertion_quantile if mode == "insertion" else an.deletion_quantile
    assert got_q == ref_q and len(got_q) == 2
    assert (an.deletion_quantile if mode == "insertion" else an.insertion_quantile) == []
    assert len(outs) == 3
    for i, (o, r) in enumerate(zip(outs, ref_outs)):
        assert o[2] is gw[i] or np.array_equal(o[2], gw[i])
        if r[1] is None:
            assert i == 2 and o[0] == (None, None, None) and o[1] is None and o[3][0] is None and np.isnan(o[3][1])
            continue
        probs, ci = o[3]
        logits = np.sort(np.log(r[3][0]), axis=1)
        assert (logits[:, -1] - logits[:, -2]).min() >= C.E2E_MARGIN   # log-probabilities differ as the logits do
        assert ci == r[3][1] and probs.shape == r[3][0].shape
        dp = float(np.abs(probs - r[3][0]).max())
        WORST["dp"] = max(WORST["dp"], dp)
        assert dp <= 1e-4, (i, dp)
        assert np.array_equal(o[1], r[1])
        for im, want in zip(o[0], r[0]):
            assert isinstance(im, Image.Image) and im.size == (C.E2E_SIZE, C.E2E_SIZE) and im.mode == "RGB"
            mx, share = R.u8_compare(np.asarray(im), want)
            WORST["share"] = max(WORST["share"], share)
            assert mx <= 1 and share <= R.CAP, (i, mx, share)
    # label 3 is predicted in the middle only: the chosen index is neither end
    assert 0 < outs[1][3][1] < len(qs) - 1


def test_eval_batch_does_not_change_the_results(L):
    """eval_batch below len(qs) (quantile chunks of one image: 3 + 3 + 1) and below N * len(qs) (one image
    per forward) against one chunk. Everything the project computes is compared exactly: the model inputs
    of all forwards, concatenated, are bit-equal, and so are indices, masks and image bytes. The model's
    forward is not the project's: the convolution library chooses its algorithm by batch size (21, 7, 3
    or 1 rows here), so the logits of the same input may differ in the last float32 bits; the
    probabilities get 1e-6 for that, a hundredth of the parity bar, and only for that."""
    qs = list(C.E2E_QS)
    runs, inputs, forwards = [], [], []
    for eb in (520, 3, 10):
        an, x, _ = make_analyzer(eval_batch=eb)
        model, seen = an.model, []
        an.model = lambda t, model=model, seen=seen: seen.append(t.clone()) or model(t)
        runs.append(an.isolate_necessary_components(x, list(C.E2E_LABELS), qs, mode="insertion"))
        inputs.append(torch.cat(seen))
        forwards.append([t.shape[0] for t in seen])
    assert forwards == [[21], [3, 3, 1] * 3, [7, 7, 7]]
    for other in inputs[1:]:
        assert torch.equal(inputs[0].view(torch.int32), other.view(torch.int32))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            if a[1] is None:
                assert b[1] is None
                continue
            assert a[3][1] == b[3][1] and np.abs(a[3][0] - b[3][0]).max() <= 1e-6
            assert np.array_equal(a[1], b[1])
            assert all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a[0], b[0]))


def test_map_count_is_checked_before_any_launch(L):
    """grad_wams cached from a smaller batch: isolate_necessary_components raises the reference's
    IndexError and launches nothing (no kernel record); isolate_scales stops at the shorter of the two,
    as the reference's zip does; surplus maps are left unused."""
    from wam_amd.plan import timing_drain, timing_enable
    an, x, gw = make_analyzer()
    an.grad_wams = gw[:2]
    timing_enable(True)
    timing_drain()
    try:
        with pytest.raises(IndexError, match="2 maps for 3 images"):
            an.isolate_necessary_components(x, list(C.E2E_LABELS), list(C.E2E_QS), mode="insertion")
        assert timing_drain() == []
    finally:
        timing_enable(False)
    assert len(an.isolate_scales(x, list(C.E2E_LABELS), EPS=C.EPS)) == 2
    full, _, _ = make_analyzer()   # three maps, two images: the first two maps are used
    got = full.isolate_necessary_components(x[:2], list(C.E2E_LABELS)[:2], list(C.E2E_QS), mode="insertion")
    want = an.isolate_necessary_components(x[:2], list(C.E2E_LABELS)[:2], list(C.E2E_QS), mode="insertion")
    assert len(got) == len(want) == 2 and full.grad_wams.shape[0] == 3
    for a, b in zip(got, want):
        assert a[3][1] == b[3][1] and np.array_equal(a[1], b[1]) and np.array_equal(a[3][0], b[3][0])


def test_minmax_equals_eval2d_quantisation(L):
    """normalize='minmax' at 224^2: the model inputs equal Eval2DWAM's quantisation of the same masked
    reconstruction (the mask applied through wam_coeff_masks)."""
    import wam_amd
    size, J, seed = 224, 3, 22401
    img, wam = C.make_image(size, seed), C.make_map(size, seed)
    x = torch.tensor(np.moveaxis(img, 2, 0)[None])
    an = wam_amd.WAMAnalyzer2D(testmodels.TinySmooth2D().cuda(), wavelet="haar", J=J, normalize="minmax")
    an.grad_wams = wam[None]
    seen = []
    model = an.model
    an.model = lambda t: seen.append(t.clone()) or model(t)
    an.isolate_necessary_components(x, [0], [0.9, 0.3], mode="insertion")
    ev = wam_amd.Eval2DWAM(model, wavelet="haar", J=J)
    masks = torch.tensor(np.stack([wam >= np.quantile(wam, q) for q in (0.9, 0.3)]).astype(np.float32)).cuda()
    want = ev._altered_inputs(ev._images(x)[0], masks)
    assert len(seen) == 1 and torch.equal(seen[0], want)


def test_user_transform_receives_pil_images(L):
    seen = []

    def tf(im):
        seen.append((type(im).__name__, im.size, im.mode))
        return torch.tensor(np.asarray(im, dtype=np.float32)).permute(2, 0, 1) / 255.0

    an, x, _ = make_analyzer()
    outs = an.isolate_necessary_components(x, list(C.E2E_LABELS), list(C.E2E_QS), transform=tf, mode="insertion")
    assert len(outs) == 3 and len(seen) == 3 * len(C.E2E_QS)
    assert set(seen) == {("Image", (C.E2E_SIZE, C.E2E_SIZE), "RGB")}


def test_isolate_scales_batches_the_module_function(L):
    from wam_amd.analysis import generate_disentangled_images
    an, x, gw = make_analyzer()
    outs = an.isolate_scales(x, list(C.E2E_LABELS), EPS=C.EPS)
    assert len(outs) == 3
    for i, (images, filtered) in enumerate(outs):
        assert images.shape == (C.E2E_J + 1, C.E2E_SIZE, C.E2E_SIZE, 3) and images.dtype == np.float64
        want_i, want_f = generate_disentangled_images(gw[i], R.show(x[i]), C.E2E_J, EPS=C.EPS)
        assert np.array_equal(images, want_i) and np.array_equal(filtered, want_f)


def test_constructor_keeps_the_reference_wiring(L):
    import wam_amd
    an = wam_amd.WAMAnalyzer2D(testmodels.TinySmooth2D().cuda(), "haar", 3, None, "reflect", False, "integratedgrad", 7,
                               0.5, 1)
    assert an.method == "smooth" and an.smooted_grad_wam.method == "integratedgrad"
    assert (an.n_samples, an.stdev_spread, an.random_seed) == (7, 0.5, 1)
    assert (an.smooted_grad_wam.n_samples, an.smooted_grad_wam.stdev_spread, an.smooted_grad_wam.random_seed) == (25, 0.25, 42)
    assert an.grad_wams is None and an.insertion_quantile == [] and an.deletion_quantile == []
    with pytest.raises(ValueError):
        wam_amd.WAMAnalyzer2D(testmodels.TinySmooth2D().cuda(), normalize="other")


def test_grad_wams_are_computed_once_and_cached(L):
    import wam_amd
    an = wam_amd.WAMAnalyzer2D(testmodels.TinySmooth2D().cuda(), wavelet="haar", J=3, n_samples=2)
    an.smooted_grad_wam.n_samples = 2
    calls = []
    inner = an.smooted_grad_wam
    an.smooted_grad_wam = lambda *a: calls.append(1) or inner(*a)
    x = torch.tensor(np.random.RandomState(1).standard_normal((1, 3, 224, 224)).astype(np.float32))
    an.isolate_necessary_components(x, [8], [0.9, 0.0], mode="insertion")
    gw = an.grad_wams
    an.isolate_scales(x, [8])
    assert len(calls) == 1 and an.grad_wams is gw and gw.shape == (1, 224, 224)


def test_errors(L):
    import wam_amd
    x = torch.rand(1, 3, 224, 224)
    an = wam_amd.WAMAnalyzer2D(testmodels.TinySmooth2D().cuda(), wavelet="db4", J=3)
    an.grad_wams = np.random.RandomState(0).uniform(size=(1, 224, 224))
    with pytest.raises(ValueError, match=r"\(244,244\) \(224,224\)"):
        an.isolate_necessary_components(x, [0], [0.9, 0.5], mode="insertion")
    with pytest.raises(ValueError):
        an.isolate_scales(x, [0])
    an, x, _ = make_analyzer()
    with pytest.raises(ValueError):
        an.isolate_necessary_components(x, list(C.E2E_LABELS), [0.9, 0.5])
    with pytest.raises(ValueError, match="insertion"):
        an.isolate_necessary_components(x, list(C.E2E_LABELS), [0.9, 0.5], mode="removal")
    with pytest.raises(AssertionError):
        an.isolate_necessary_components(x, list(C.E2E_LABELS), [0.5, 0.9], mode="insertion")
    with pytest.raises(AssertionError):
        an.isolate_necessary_components(x, list(C.E2E_LABELS), [0.9, 0.5], mode="deletion")
    an.grad_wams = np.zeros((3, 64, 32))
    with pytest.raises(ValueError):
        an.isolate_necessary_components(x, list(C.E2E_LABELS), [0.9, 0.5], mode="insertion")
