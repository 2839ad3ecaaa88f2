"""Pixel-domain baselines on the GPU (wam_amd/csrc/baselines2d.hip, wam_amd/baselines.py) against the
numpy restatement (tests/baselines_ref.py, pinned to the reference's goldens by tests/test_baselines_ref.py)
and against the goldens themselves.

Bars: the two mask entries and the channel mean are bit for bit (every operation is a single IEEE
float32 one). The CAMs are held to 4 * D_CAM relative to the map's maximum (D_CAM: the float64
restatement against the reference's float32 loop; 4: the project's device margin); the device sums in
float64 too, so what it leaves at the C ABI is the final float32 rounding. Measured on one MI355X (the
worst of both is printed when the module finishes): 1.21e-7 to the restatement at the C ABI; to the
goldens through the GPU model 3.8e-7 to 5.6e-7 for six of the eight (method, layer, size) cases, 9.06e-7
for gradcam / conv2 / 64^2 and 1.347e-6 for gradcam / conv2 / 32^2 -- the float32 convolutions of another
backend under the map's min-max normalisation; the same figures in three runs. Everything else that goes
through the model is held to 1e-4, mu-fidelity to 0.05 (tests/test_gpu_eval.py's bars).
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests import baselines_ref as R
from tests.analyzer_ref import assert_bits
from tests.golden import imgbase_cases as C
from tests.helpers import npz

pytestmark = pytest.mark.gpu

MEAN, STD = R.IMAGENET_MEAN, R.IMAGENET_STD
_WORST = {"cam": 0.0}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    yield _lib
    print("\n[test_gpu_baselines] worst CAM distance to the restatement / goldens: %.3e (bar %.1e)"
          % (_WORST["cam"], 4 * R.D_CAM))


def G():
    return npz(C.GOLDENS)


def _consts(L, C_):
    return (L.c_f32 * C_)(*MEAN[:C_]), (L.c_f32 * C_)(*STD[:C_])


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _ranks(rs, sets, P):
    return np.stack([rs.permutation(P) for _ in range(sets)]).astype(np.int32)


def _rank_call(L, img, rank, n_iter, n_comp, deletion, want=("masked", "u8", "out"), shift=0):
    """wam_rank_mask_pixels on device copies of img / rank; shift = 1 moves every float / int base by one
    element (and the bytes by one byte): the scalar path."""
    sets, C_, P = img.shape
    n = sets * (n_iter + 1) * C_ * P

    def buf(a):
        t = torch.empty(a.size + shift, dtype=torch.as_tensor(a).dtype, device="cuda")
        t[shift:] = torch.as_tensor(np.ascontiguousarray(a)).reshape(-1)
        return t

    d_img, d_rank = buf(img), buf(rank)
    outs = {"masked": torch.full((n + shift,), 7.0, dtype=torch.float32, device="cuda"),
            "u8": torch.full((n + shift,), 7, dtype=torch.uint8, device="cuda"),
            "out": torch.full((n + shift,), 7.0, dtype=torch.float32, device="cuda")}
    ws = torch.empty(int(L.lib.wam_rank_mask_pixels_ws_bytes(sets, n_iter)) // 4, dtype=torch.float32, device="cuda")
    mean, std = _consts(L, C_)

    def p(t):
        return ctypes.c_void_p(t.data_ptr() + shift * t.element_size())

    rc = L.lib.wam_rank_mask_pixels(sets, C_, P, p(d_img), p(d_rank), n_iter, n_comp, int(deletion), mean, std,
                                    p(outs["masked"]) if "masked" in want else None,
                                    p(outs["u8"]) if "u8" in want else None,
                                    p(outs["out"]) if "out" in want else None, L.ptr(ws), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    shape = (sets * (n_iter + 1), C_, P)
    got = {k: (v[shift:].cpu().numpy().reshape(shape) if k in want else None) for k, v in outs.items()}
    for k, v in outs.items():  # nothing outside the outputs, and no output that was not asked for, is written
        if k not in want:
            assert bool((v == 7).all()), k
        elif shift:
            assert float(v[0]) == 7
    return got


def _check_rank(L, img, rank, n_iter, deletion, what, **kw):
    P = img.shape[2]
    n_comp = int(P / n_iter)
    masked, u8, out = R.rank_mask_pixels_ref(img, rank, n_iter, n_comp, deletion, MEAN[:img.shape[1]],
                                             STD[:img.shape[1]])
    got = _rank_call(L, img, rank, n_iter, n_comp, deletion, **kw)
    for k, ref in (("masked", masked), ("u8", u8), ("out", out)):
        if got[k] is not None:
            assert_bits(got[k], ref, "%s %s" % (what, k))
    return got


# --------------------------------------------------------------------------------- entry (a)
@pytest.mark.parametrize("hw", [(15, 17), (5, 4), (96, 96), (224, 224)])
@pytest.mark.parametrize("deletion", [False, True])
def test_rank_mask_pixels_bits(L, hw, deletion):
    P = hw[0] * hw[1]
    rs = np.random.RandomState(P + int(deletion))
    for C_ in (1, 3):
        for sets in (1, 3):
            img = rs.standard_normal((sets, C_, P)).astype(np.float32)   # negative pixels
            for n_iter in ((7, 8, 32) if P == 20 else (7, 8)):
                _check_rank(L, img, _ranks(rs, sets, P), n_iter, deletion, "%s C%d s%d n%d" % (hw, C_, sets, n_iter))


@pytest.mark.parametrize("hw", [(15, 17), (96, 96)])
def test_rank_mask_pixels_outputs_alone_and_unaligned(L, hw):
    P = hw[0] * hw[1]
    rs = np.random.RandomState(P)
    img = rs.standard_normal((2, 3, P)).astype(np.float32)
    rank = _ranks(rs, 2, P)
    for want in (("masked",), ("u8",), ("out",)):
        _check_rank(L, img, rank, 7, False, "alone", want=want)
    _check_rank(L, img, rank, 7, True, "one element off", shift=1)   # 96 x 96: P % 4 == 0, pointers unaligned


def test_rank_mask_pixels_out_is_quantize_of_masked(L):
    rs = np.random.RandomState(5)
    P = 96 * 96
    img = rs.standard_normal((2, 3, P)).astype(np.float32)
    got = _rank_call(L, img, _ranks(rs, 2, P), 8, int(P / 8), True)
    n = got["masked"].shape[0]
    masked = _dev(got["masked"])
    out = torch.empty_like(masked)
    u8 = torch.empty(masked.shape, dtype=torch.uint8, device="cuda")
    mean, std = _consts(L, 3)
    L.check(L.lib.wam_quantize_normalize_ex(n, 3, P, L.ptr(masked), 0, mean, std, L.ptr(u8), L.ptr(out), None))
    assert_bits(got["out"], out.cpu().numpy(), "out")
    assert_bits(got["u8"], u8.cpu().numpy(), "u8")


def test_rank_mask_pixels_constant_images(L):
    """A constant image: the full and the empty mask have equal extrema, 0 / 0 = NaN -> byte 0; an all-zero
    image: every mask does."""
    rs = np.random.RandomState(6)
    P = 15 * 17
    img = np.stack([np.full((3, P), 0.25), np.zeros((3, P)), np.full((3, P), -1.5)]).astype(np.float32)
    for deletion in (False, True):
        got = _check_rank(L, img, _ranks(rs, 3, P), 8, deletion, "constant")
        u8 = got["u8"].reshape(3, 9, 3, P)
        assert not u8[0, 0].any() and not u8[0, 8].any() and not u8[1].any()
        assert u8[0, 1:8].any()


def test_rank_mask_pixels_bound_and_arguments(L):
    img = torch.zeros(3 * 16, device="cuda")
    rank = torch.zeros(16, dtype=torch.int32, device="cuda")
    out = torch.full((4098 * 3 * 16,), 7.0, device="cuda")
    ws = torch.empty(int(L.lib.wam_rank_mask_pixels_ws_bytes(1, 4097)) // 4, device="cuda")
    mean, std = _consts(L, 3)
    args = lambda n_iter, o=out, w=ws: (1, 3, 16, L.ptr(img), L.ptr(rank), n_iter, 0, 0, mean, std, None, None,  # noqa: E731
                                        L.ptr(o) if o is not None else None, L.ptr(w) if w is not None else None, None)
    assert L.lib.wam_rank_mask_pixels(*args(4097)) == 3            # WAM_ERR_UNSUPPORTED, one above the bound
    assert L.lib.wam_rank_mask_pixels(*args(0)) == 1
    assert L.lib.wam_rank_mask_pixels(*args(8, o=None)) == 1       # no output
    assert L.lib.wam_rank_mask_pixels(*args(8, w=None)) == 1       # no workspace
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert L.lib.wam_rank_mask_pixels(*args(4096)) == 0            # the bound itself runs
    torch.cuda.synchronize()
    assert bool((out[:4097 * 3 * 16] != 7).all()) and bool((out[4097 * 3 * 16:] == 7).all())


# --------------------------------------------------------------------------------- entry (b)
def _cell_call(L, img, grid, cell):
    C_, P = img.shape
    n = grid.shape[0]
    d_img, d_grid, d_cell = _dev(img), _dev(grid), _dev(cell.astype(np.int32))
    masked = torch.empty((n, C_, P), dtype=torch.float32, device="cuda")
    u8 = torch.empty((n, C_, P), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, C_, P), dtype=torch.float32, device="cuda")
    mean, std = _consts(L, C_)
    L.check(L.lib.wam_cell_mask_pixels(C_, P, L.ptr(d_img), n, grid.shape[1], L.ptr(d_grid), L.ptr(d_cell), mean, std,
                                       L.ptr(masked), L.ptr(u8), L.ptr(out), None))
    return masked.cpu().numpy(), u8.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("size", [64, 224])
@pytest.mark.parametrize("grid_size", [8, 28])
def test_cell_mask_pixels_bits(L, size, grid_size):
    from wam_amd.evaluation import zoom_cell_map
    rs = np.random.RandomState(size + grid_size)
    cell = zoom_cell_map(grid_size, (size, size)).reshape(-1)
    for C_, n in ((3, 16), (1, 1)):
        img = rs.standard_normal((C_, size * size)).astype(np.float32)
        grid = rs.uniform(size=(n, grid_size * grid_size)).astype(np.float32)
        if n == 16:
            grid[3] = 1.0    # all ones: the image itself
            grid[5] = 0.0    # all zeros: a constant image, NaN -> byte 0
        got = _cell_call(L, img, grid, cell)
        ref = R.cell_mask_pixels_ref(img, grid, cell, MEAN[:C_], STD[:C_])
        for k, a, b in zip(("masked", "u8", "out"), got, ref):
            assert_bits(a, b, "C%d n%d %s" % (C_, n, k))
        if n == 16:
            assert not got[1][5].any()


def test_cell_mask_pixels_scalar_path(L):
    """A plane that is no multiple of 4 (15 x 17 pixels on a 5 x 5 grid)."""
    from wam_amd.evaluation import zoom_cell_map
    rs = np.random.RandomState(2)
    cell = zoom_cell_map(5, (15, 17)).reshape(-1)
    img = rs.standard_normal((3, 255)).astype(np.float32)
    grid = rs.uniform(size=(4, 25)).astype(np.float32)
    for k, a, b in zip(("masked", "u8", "out"), _cell_call(L, img, grid, cell),
                       R.cell_mask_pixels_ref(img, grid, cell, MEAN, STD)):
        assert_bits(a, b, k)


# --------------------------------------------------------------------------------- entry (c)
def _cam_call(L, act, grad, pp, size):
    from wam_amd.baselines import cam_maps
    return cam_maps(_dev(act), _dev(grad), pp, size).cpu().numpy()


@pytest.mark.parametrize("shape", [(2, 1, 4, 4, 8, 8), (2, 5, 3, 4, 17, 23), (3, 8, 16, 16, 32, 32),
                                   (2, 2048, 7, 7, 224, 224), (2, 3, 8, 8, 8, 8), (2, 4, 40, 40, 64, 64)])
@pytest.mark.parametrize("pp", [False, True])
def test_cam_maps_vs_restatement(L, shape, pp):
    N, K, h, w, oh, ow = shape
    rs = np.random.RandomState(K + h)
    act = rs.uniform(-0.2, 1.0, size=(N, K, h, w)).astype(np.float32)
    grad = rs.standard_normal((N, K, h, w)).astype(np.float32)
    grad[0] = np.abs(grad[0])          # image 0: a CAM that is positive somewhere for sure
    act[0] = np.abs(act[0])
    got = _cam_call(L, act, grad, pp, (oh, ow))
    ref = R.cam_maps_ref(act, grad, pp, (oh, ow))
    assert np.isfinite(ref[0]).all()
    d = R.cam_distance(got, ref)
    _WORST["cam"] = max(_WORST["cam"], d)
    assert d <= 4 * R.D_CAM, d


def test_cam_maps_nowhere_positive_is_nan_everywhere(L):
    rs = np.random.RandomState(1)
    act = rs.uniform(0.1, 1.0, size=(2, 6, 5, 5)).astype(np.float32)
    grad = -rs.uniform(0.1, 1.0, size=(2, 6, 5, 5)).astype(np.float32)
    grad[1] = -grad[1]
    got = _cam_call(L, act, grad, False, (20, 20))
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()
    d = _dev(act)   # 8 * (K + h * w + 1040) bytes of LDS: K = 30000 is declined before anything is read
    assert L.lib.wam_cam_maps(1, 30000, 7, 7, L.ptr(d), L.ptr(d), 0, 8, 8, L.ptr(d), None) == 3


# --------------------------------------------------------------------------------- entry (d)
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_channel_mean_bits(L, C_):
    rs = np.random.RandomState(C_)
    g = rs.standard_normal((3, C_, 15 * 17)).astype(np.float32)
    m = rs.standard_normal((3, C_, 15 * 17)).astype(np.float32)
    base = rs.standard_normal((3, 15 * 17))
    for mult in (None, m):
        for absolute in (False, True):
            ref = R.channel_mean_ref(g, mult, absolute)
            out = torch.empty((3, 255), dtype=torch.float32, device="cuda")
            acc, d_g, d_mult = _dev(base), _dev(g), (_dev(mult) if mult is not None else None)
            L.check(L.lib.wam_channel_mean(3, C_, 255, L.ptr(d_g), L.ptr(d_mult), int(absolute), L.ptr(out), L.ptr(acc),
                                           None))
            assert_bits(out.cpu().numpy(), ref, "out_f32")
            assert_bits(acc.cpu().numpy(), base + ref.astype(np.float64), "acc_f64")
    if C_ == 3:
        want = np.mean(np.transpose(g.reshape(3, 3, 15, 17), (0, 2, 3, 1)), axis=-1)
        assert_bits(R.channel_mean_ref(g).reshape(3, 15, 17), want, "numpy's mean")


# --------------------------------------------------------------------------------- methods
def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


@pytest.mark.parametrize("size", C.CAM_SIZES)
@pytest.mark.parametrize("layer", C.CAM_LAYERS)
def test_cam_classes_vs_goldens(L, size, layer):
    from wam_amd.baselines import GradCAM, GradCAMPlusPlus
    x, y = C.cam_inputs(size)
    for name, cls in (("gradcam", GradCAM), ("gradcampp", GradCAMPlusPlus)):
        model = C.make_model().cuda()
        got = cls(model, getattr(model, layer))(x, y)
        ref = G()["cam_%s_%s_%d" % (name, layer, size)]
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert not model._forward_hooks and not getattr(model, layer)._forward_hooks
        d = R.cam_distance(got, ref)    # the golden's all-NaN map must be NaN everywhere here too
        print("%s %s %d: distance to the golden %.3e" % (name, layer, size, d))
        _WORST["cam"] = max(_WORST["cam"], d)
        assert d <= 4 * R.D_CAM, (name, d)


def test_smoothgrad(L):
    from wam_amd.baselines import SmoothGrad, channel_mean
    x, y = C.cam_inputs(32)
    model = C.make_model().cuda()
    sg = SmoothGrad(model, n_samples=3, random_seed=11)
    got = sg(x, y)
    assert got.dtype == np.float64 and got.shape == (3, 32, 32)
    assert np.array_equal(got, SmoothGrad(model, n_samples=3, random_seed=11)(x, y))      # deterministic per seed
    assert not np.array_equal(got, SmoothGrad(model, n_samples=3, random_seed=12)(x, y))
    noisy = [sg.noisy(x.cuda(), s).cpu().numpy() for s in range(3)]
    assert np.abs(noisy[0] - x.numpy()).max() > 0.05 and not np.array_equal(noisy[0], noisy[1])
    assert _rel(got, R.smoothgrad_ref(C.make_model(), x, y, noisy)) < 1e-4
    # no noise, one sample: the plain gradient's channel mean (the convolution's backward may sum in
    # another order from call to call: rounding, not bits)
    plain = SmoothGrad(model, n_samples=1, stdev_spread=0.0)(x, y)
    xs = x.cuda().requires_grad_(True)
    loss = torch.diag(model(xs)[:, torch.tensor(y).cuda()]).mean()
    want = channel_mean(torch.autograd.grad(loss, xs)[0]).cpu().numpy()
    assert _rel(plain, want) < 1e-6


def test_saliency_and_integrated_gradients(L):
    from wam_amd.baselines import IntegratedGradients, Saliency
    x, y = C.cam_inputs(32)
    model = C.make_model().cuda()
    sal = Saliency(model)
    attr = sal.attribute(x, target=torch.tensor(y))
    assert tuple(attr.shape) == (3, 3, 32, 32) and bool((attr >= 0).all())
    assert _rel(sal.maps(x, y).cpu().numpy(), R.saliency_ref(C.make_model(), x, y)) < 1e-4
    ig = IntegratedGradients(model)
    ref = R.integrated_gradients_ref(C.make_model(), x, y, n_steps=50)
    got = ig.attribute(x, target=torch.tensor(y), method="riemann_trapezoid", n_steps=50, internal_batch_size=2)
    assert tuple(got.shape) == (3, 3, 32, 32) and _rel(got.cpu().numpy(), ref) < 1e-4
    whole, delta = ig.attribute(x, target=y, n_steps=50, return_convergence_delta=True)
    assert _rel(whole.cpu().numpy(), ref) < 1e-4 and tuple(delta.shape) == (3,) and float(delta.abs().max()) < 1e-2
    maps = ig.maps(x, y, internal_batch_size=64).cpu().numpy()
    assert _rel(maps, R.channel_mean_ref(ref.astype(np.float32).reshape(3, 3, -1)).reshape(3, 32, 32)) < 1e-4
    with pytest.raises(ValueError):
        ig.attribute(x, target=y, method="gausslegendre")


# --------------------------------------------------------------------------------- the class
def _evaluator(method="saliency", **kw):
    from wam_amd.evaluation import EvalImageBaselines
    model = C.make_model().cuda()
    seen = []
    model.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().cpu().numpy().copy()))
    return EvalImageBaselines(method, model, **kw), seen


@pytest.mark.parametrize("name", sorted(C.CLASS_CASES))
@pytest.mark.parametrize("mode", C.MODES)
def test_insertion_deletion_vs_goldens(L, name, mode):
    """c224: the fused output; c64: masked floats through the Pillow-exact resize. The stored rows of
    image 0's model inputs are the reference's bit for bit."""
    case = C.CLASS_CASES[name]
    x, y, expl = C.class_inputs(case)
    ev, seen = _evaluator()
    ev.explanations = expl
    ev.compute_explanations = None   # the cache is honoured: nothing may call this
    scores = getattr(ev, mode)(x, y, n_iter=case["n_iter"])
    curves = ev.insertion_curves if mode == "insertion" else ev.deletion_curves
    g = G()
    inputs = np.concatenate(seen)
    assert inputs.shape == (2 * (case["n_iter"] + 1), 3, 224, 224)
    assert_bits(np.stack([C.digest(inputs[r]) for r in case["rows"]]), g["%s_%s_inputs" % (name, mode)], "model inputs")
    assert np.abs(np.array(scores) - g["%s_%s_scores" % (name, mode)]).max() < 1e-4
    assert np.abs(np.array(curves) - g["%s_%s_curves" % (name, mode)]).max() < 1e-4
    assert ev.explanations is expl


def test_saliency_end_to_end_vs_goldens(L):
    case = C.SAL_CASE
    x, y, _ = C.class_inputs(case)
    ev, _ = _evaluator()
    g = G()
    for mode in C.MODES:
        scores = getattr(ev, mode)(x, y, n_iter=case["n_iter"])
        curves = ev.insertion_curves if mode == "insertion" else ev.deletion_curves
        assert np.abs(np.array(scores) - g["sal_%s_scores" % mode]).max() < 1e-4
        assert np.abs(np.array(curves) - g["sal_%s_curves" % mode]).max() < 1e-4
    assert ev.explanations.dtype == np.float32 and _rel(ev.explanations, g["sal_expl"]) < 1e-4


def test_mu_fidelity_vs_goldens(L, monkeypatch):
    import wam_amd.baselines as B
    case = C.MU_CASE
    x, y, expl = C.class_inputs(case)
    ev, _ = _evaluator(batch_size=case["batch_size"])
    ev.explanations = expl
    pairs, masks = [], []
    real = B.spearmanr
    monkeypatch.setattr(B, "spearmanr", lambda a, b: (pairs.append((np.array(a), np.array(b))), real(a, b))[1])
    inner = ev.compute_baseline_state
    ev.compute_baseline_state = lambda *a: (masks.append(inner(*a)), masks[-1])[1]
    random.seed(case["pyseed"])
    mu = ev.mu_fidelity(x, y, grid_size=case["grid_size"], sample_size=case["sample_size"],
                        subset_size=case["subset_size"])
    g = G()
    assert len(mu) == len(pairs) == len(masks) == 2
    for i in range(2):
        assert_bits(masks[i], g["mu_bmask"][i], "baseline mask")
        assert np.abs(pairs[i][0] - g["mu_preds"][i]).max() < 1e-4
        assert np.abs(pairs[i][1] - g["mu_attrs"][i]).max() <= 1e-6 * np.abs(g["mu_attrs"][i]).max()
    assert np.abs(np.array(mu) - g["mu_value"]).max() < 0.05


def test_user_transform_receives_pil_images(L):
    seen = []

    def tf(im):
        seen.append((type(im).__name__, im.size, im.mode))
        return torch.tensor(np.asarray(im, dtype=np.float32)).permute(2, 0, 1) / 255.0

    from wam_amd.evaluation import EvalImageBaselines
    ev = EvalImageBaselines("saliency", C.make_model().cuda(), transform=tf)
    x, y, expl = C.class_inputs(C.CLASS_CASES["c64"])
    ev.explanations = expl
    scores = ev.insertion(x, y, n_iter=4)
    assert len(scores) == 2 and len(seen) == 10 and seen[0] == ("Image", (64, 64), "RGB")


def test_names(L):
    from wam_amd.evaluation import EvalImageBaselines
    model = C.make_model().cuda()
    for name in ("guided_backprop", "layercam", "lrp", "srd"):
        with pytest.raises(NotImplementedError):
            EvalImageBaselines(name, model)
    with pytest.raises(ValueError):
        EvalImageBaselines("occlusion", model)
    with pytest.raises(RuntimeError):
        EvalImageBaselines("saliency", C.make_model())   # a CPU model: the kernels run on the GPU only
    for name, cls in (("gradcam", "GradCAM"), ("gradcampp", "GradCAMPlusPlus"), ("smoothgrad", "SmoothGrad"),
                      ("integratedgrad", "IntegratedGradients")):
        assert type(EvalImageBaselines(name, model, layers=model.conv2).method).__name__ == cls
