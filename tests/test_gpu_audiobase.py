"""wam_cam_maps_tiled (wam_amd/csrc/cam_tiled.hip) and EvalAudioBaselines (wam_amd/baselines_audio.py) on
the GPU, against the numpy references (tests/baselines_ref.py cam_maps_ref, tests/audiobase_ref.py,
tests/eval1d_ref.py rank_mask_rows_ref) and the goldens made by the reference's own class
(tests/golden/audiobase_goldens.npz).

Bars. The tiled CAM at the C ABI: 4 * D_CAM relative to the map's maximum (D_CAM: the float64 restatement
against the reference's float32 loop; 4: the project's device margin); the device sums in float64 too, so
what it leaves is the final float32 rounding. Masked rows: bit for bit. Everything that passes through the
model on another backend -- explanations against the goldens, class probabilities, scores, faithfulness
of spectra -- 1e-4 (tests/eval1d_ref.py BAR; the same device pipeline as Eval1DWAM's mel target).

Grad-CAM at n_iter = 7 ranks runs of exact ReLU zeros across thresholds, and one cell that is zero on one
backend and 1e-9 on the other moves a whole dB cell of a masked input: that comparison runs the restatement
(stable sort) on the explanation the device class computed, so that it checks the tie order and the
pipeline, not the backend's last bit.

Measured on one MI355X (printed when the module finishes; each test prints its own figure): the tiled CAM
against the restatement at the C ABI 1.21e-7 at worst (0 on ten of the twelve shape / method cases), against
wam_cam_maps at the in-bound shapes 7.6e-9; the large-map Grad-CAM through the class 0 to the restatement on
the device's own layer tensors and 5.36e-7 to the golden; explanations against the goldens 5.44e-6
(saliency, 158 x 128), 1.11e-6 (integrated gradients), 7.45e-7 (Grad-CAM, small case); class probabilities
1.19e-7, scores 1.79e-7, faithfulness of spectra 2.98e-8. The whole module takes 6 s.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import audiobase_ref as A
from tests import baselines_ref as B
from tests import eval1d_ref as R1
from tests.golden import audiobase_cases as C

pytestmark = pytest.mark.gpu
CAM_BAR = 4 * B.D_CAM
WORST = {"cam_abi": 0.0, "cam_vs_lds": 0.0, "cam_big_own": 0.0, "cam_big_golden": 0.0, "expl": 0.0, "cam_small": 0.0,
         "p": 0.0, "score": 0.0, "ff": 0.0}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()
    print("\n[test_gpu_audiobase] worst distances: " + ", ".join("%s %.3e" % kv for kv in WORST.items()))


def _note(key, value):
    WORST[key] = max(WORST[key], float(value))
    return value


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


# --------------------------------------------------------------------------------- the tiled CAM at the C ABI
def _cam_inputs(N, K, h, w):
    rs = np.random.RandomState(K + h)
    act = rs.uniform(-0.2, 1.0, size=(N, K, h, w)).astype(np.float32)
    grad = rs.standard_normal((N, K, h, w)).astype(np.float32)
    grad[0] = np.abs(grad[0])          # image 0: a CAM that is positive somewhere for sure
    act[0] = np.abs(act[0])
    return act, grad


def _tiled_call(L, act, grad, pp, size, shift=0):
    """wam_cam_maps_tiled on device copies; shift = 1 moves act, grad and out by one float and ws by one
    double: the scalar load path. Nothing outside out is written."""
    N, K, h, w = act.shape
    n_out = N * size[0] * size[1]

    def buf(a):
        t = torch.empty(a.size + shift, dtype=torch.float32, device="cuda")
        t[shift:] = torch.as_tensor(np.ascontiguousarray(a)).reshape(-1)
        return t

    d_act, d_grad = buf(act), buf(grad)
    out = torch.full((n_out + shift + 1,), 7.0, dtype=torch.float32, device="cuda")
    nbytes = int(L.lib.wam_cam_maps_tiled_ws_bytes(N, K, h, w))
    ws = torch.empty(nbytes // 8 + shift, dtype=torch.float64, device="cuda")

    def p(t):
        return ctypes.c_void_p(t.data_ptr() + shift * t.element_size())

    if shift:
        assert (d_act.data_ptr() + 4) % 16 != 0
    rc = L.lib.wam_cam_maps_tiled(N, K, h, w, p(d_act), p(d_grad), int(pp), size[0], size[1], p(out), p(ws), nbytes,
                                  L.stream_of(out.device))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert float(out[-1]) == 7 and (not shift or float(out[0]) == 7)
    return out[shift:shift + n_out].cpu().numpy().reshape(N, size[0], size[1])


TILED_SHAPES = [(2, 4, 157, 128, 157, 128),      # c3's mel, 16-byte loads, 20 tiles, 20 splits
                (1, 3, 150, 131, 300, 262),      # odd width: scalar loads, a partial last tile
                (1, 19500, 2, 2, 8, 8),          # K alone past the LDS bound: 77 weight chunks
                (1, 16, 431, 128, 431, 128),     # the reference's ESC-50 mel: 54 tiles
                (2, 5, 3, 4, 17, 23),            # inside the LDS bound
                (2, 2048, 7, 7, 224, 224)]


@pytest.mark.parametrize("shape", TILED_SHAPES)
@pytest.mark.parametrize("pp", [False, True])
def test_tiled_cam_vs_restatement(L, shape, pp):
    N, K, h, w, oh, ow = shape
    act, grad = _cam_inputs(N, K, h, w)
    got = _tiled_call(L, act, grad, pp, (oh, ow))
    ref = B.cam_maps_ref(act, grad, pp, (oh, ow))
    assert np.isfinite(ref[0]).all()
    d = _note("cam_abi", B.cam_distance(got, ref))
    print("tiled %s pp=%d: distance to the restatement %.3e" % (shape, pp, d))
    assert d <= CAM_BAR, d
    if 8 * (K + h * w + 1040) <= 160 * 1024:
        from wam_amd.baselines import cam_maps
        lds = cam_maps(_dev(act), _dev(grad), pp, (oh, ow)).cpu().numpy()
        print("tiled %s pp=%d: distance to wam_cam_maps %.3e" % (shape, pp, _note("cam_vs_lds", B.cam_distance(got, lds))))


@pytest.mark.parametrize("pp", [False, True])
def test_tiled_cam_unaligned_pointers_same_values(L, pp):
    """Every base pointer one element off: the scalar path at a shape the 16-byte path serves. Within the
    bar of the restatement, and the same bits as the aligned call."""
    act, grad = _cam_inputs(2, 4, 157, 128)
    ref = B.cam_maps_ref(act, grad, pp, (157, 128))
    aligned = _tiled_call(L, act, grad, pp, (157, 128))
    shifted = _tiled_call(L, act, grad, pp, (157, 128), shift=1)
    assert _note("cam_abi", B.cam_distance(shifted, ref)) <= CAM_BAR
    R1.assert_bits(shifted, aligned, "scalar path vs 16-byte path")


def test_tiled_cam_nowhere_positive_is_nan_everywhere(L):
    rs = np.random.RandomState(1)
    act = rs.uniform(0.1, 1.0, size=(2, 3, 150, 131)).astype(np.float32)
    grad = -rs.uniform(0.1, 1.0, size=(2, 3, 150, 131)).astype(np.float32)
    grad[1] = -grad[1]
    got = _tiled_call(L, act, grad, False, (75, 140))
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()
    assert B.cam_distance(got, B.cam_maps_ref(act, grad, False, (75, 140))) <= CAM_BAR


def test_tiled_cam_two_calls_equal_bits(L):
    act, grad = _cam_inputs(2, 16, 157, 128)
    for pp in (False, True):
        a = _tiled_call(L, act, grad, pp, (157, 128))
        b = _tiled_call(L, act, grad, pp, (157, 128))
        R1.assert_bits(a, b, "two calls")


# --------------------------------------------------------------------------------- through the classes
def _evaluator(name, method, **kw):
    from wam_amd import EvalAudioBaselines
    case = C.CASES[name]
    model = C.make_model().cuda()
    seen = []
    model.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().cpu().numpy().copy()))
    ev = EvalAudioBaselines(method, model, n_fft=case["n_fft"], sample_rate=C.SAMPLE_RATE, n_mels=case["n_mels"], **kw)
    return ev, seen


def test_gradcam_large_map_goes_through_the_tiled_route(L, monkeypatch):
    """TinyAudio.conv on the 158 x 128 mel: K + h * w = 20,228 is past wam_cam_maps' 19,440."""
    import wam_amd.baselines as WB
    from wam_amd.evalcore import db_melspec
    case = C.CASES["big20096"]
    x, y = C.make_inputs(case)
    mel = db_melspec(x.cuda(), case["n_fft"], C.SAMPLE_RATE, case["n_mels"])
    assert tuple(mel.shape) == (2, 1, 158, 128)
    calls = []
    real = WB.cam_maps_tiled
    monkeypatch.setattr(WB, "cam_maps_tiled", lambda *a: (calls.append(a[0].shape), real(*a))[1])
    model = C.make_model().cuda()
    cam = WB.GradCAM(model, model.conv)
    got = cam(mel, y)
    assert calls == [(2, 4, 158, 128)] and got.dtype == np.float32 and got.shape == (2, 158, 128)
    act, grad = cam.layer_tensors(mel, y)
    own = B.cam_maps_ref(act.cpu().numpy(), grad.cpu().numpy(), False, (158, 128))
    d_own = _note("cam_big_own", B.cam_distance(got, own))
    d_gold = _note("cam_big_golden", B.cam_distance(got, C.golden("big20096", "gradcam", "expl")))
    print("large-map Grad-CAM: %.3e to the restatement on the device's own layer tensors, %.3e to the golden"
          % (d_own, d_gold))
    assert d_own <= CAM_BAR
    assert d_gold <= 1e-4
    with pytest.raises(L.WamError):   # the old entry still declines this shape
        L.check(L.lib.wam_cam_maps(2, 4, 158, 128, L.ptr(act), L.ptr(grad), 0, 158, 128, L.ptr(act), None))


@pytest.mark.parametrize("name,method", [(n, m) for n, c in C.CASES.items() for m in c["methods"]
                                         if not (n == "big20096" and m == "gradcam")])
def test_explanations_vs_goldens(L, name, method):
    x, y = C.make_inputs(C.CASES[name])
    ev, _ = _evaluator(name, method)
    got = ev.compute_explanations(x, y)
    ref = C.golden(name, method, "expl")
    assert got.dtype == np.float32 and got.shape == ref.shape
    if method == "gradcam":
        d = _note("cam_small", B.cam_distance(got, ref))
        assert d <= 1e-4, d
    else:
        d = _note("expl", _rel(got, ref))
        assert d < 1e-4, d
    print("%s %s: explanation distance to the golden %.3e" % (name, method, d))
    assert ev.explanations is None    # computed per call, not stored


@pytest.mark.parametrize("name,method", [(n, m) for n, c in C.CASES.items() for m, it in c["methods"].items() if it])
def test_injected_explanations_vs_goldens(L, name, method):
    """Golden explanations in, tie_order='numpy': the reference's ranking, so curves, scores, FF and
    fidelity are the goldens'; the model inputs are the C-ABI reference's rows bit for bit."""
    case = C.CASES[name]
    x, y = C.make_inputs(case)
    expl = C.golden(name, method, "expl")
    ev, seen = _evaluator(name, method, tie_order="numpy")
    ev.explanations = expl
    ev.compute_explanations = None     # honoured: nothing may call this
    stable, _ = _evaluator(name, method)
    stable.explanations = expl
    source = ev._mel(x.cuda()).cpu().numpy().reshape(C.N_CLIPS, -1)
    P = source.shape[1]
    rank = np.stack([A.rank_of(A.descending_order(e)) for e in expl])
    for mode in C.MODES:
        for n_iter in case["methods"][method]:
            del seen[:]
            scores = getattr(ev, mode)(x, y, n_iter)
            curves = ev.deletion_curves if mode == "deletion" else ev.insertion_curves
            if mode == "deletion":
                assert ev.insertion_curves is ev.deletion_curves    # sic
            assert scores[0].dtype == np.float32 and curves[0].dtype == np.float32
            rows = R1.rank_mask_rows_ref(source, rank, n_iter, int(P / n_iter), mode == "deletion")
            R1.assert_bits(np.concatenate(seen).reshape(rows.shape), rows, "%s n_iter %d model inputs" % (mode, n_iter))
            dp = _note("p", np.abs(np.array(curves) - C.golden(name, method, "%s_n%d_curves" % (mode, n_iter))).max())
            ds = _note("score", np.abs(np.array(scores) - C.golden(name, method, "%s_n%d_scores" % (mode, n_iter))).max())
            assert dp <= R1.BAR and ds <= R1.BAR, (dp, ds)
            getattr(stable, mode)(x, y, n_iter)   # no straddling ties: the stable order gives the same curves
            other = stable.deletion_curves if mode == "deletion" else stable.insertion_curves
            assert np.abs(np.array(other) - np.array(curves)).max() <= R1.BAR
    dff = _note("ff", np.abs(np.array(ev.faithfulness_of_spectra(x, y)) - C.golden(name, method, "ff")).max())
    assert dff <= R1.BAR
    assert ev.input_fidelity(x, y) == C.golden(name, method, "fid").tolist()
    assert ev.explanations is expl


def test_saliency_end_to_end_vs_goldens(L):
    case = C.CASES["k4096"]
    x, y = C.make_inputs(case)
    ev, _ = _evaluator("k4096", "saliency")
    for mode in C.MODES:
        for n_iter in C.GRAD_ITERS:
            scores = getattr(ev, mode)(x, y, n_iter)
            key = "%s_n%d_" % (mode, n_iter)
            dp = _note("p", np.abs(np.array(ev.insertion_curves) - C.golden("k4096", "saliency", key + "curves")).max())
            ds = _note("score", np.abs(np.array(scores) - C.golden("k4096", "saliency", key + "scores")).max())
            assert dp <= 1e-4 and ds <= 1e-4, (dp, ds)
    assert ev.explanations is None


def test_list_input_is_peak_normalised(L):
    case = C.CASES["k4096"]
    x, y = C.make_inputs(case)
    ev, _ = _evaluator("k4096", "saliency")
    waves = [w for w in x.numpy()]
    a = ev.insertion(waves, y, 4)
    b = ev.insertion(A.peak_normalise(waves), y, 4)
    assert np.array_equal(np.array(a), np.array(b))


def test_smoothgrad(L):
    case = C.CASES["k4096"]
    x, y = C.make_inputs(case)
    ev, _ = _evaluator("k4096", "smoothgrad")
    assert ev.method.stdev_spread == 0.001 and ev.method.n_samples == 50 and ev.method.random_seed == 42
    ev.method.n_samples = 3
    got = ev.compute_explanations(x, y)
    assert got.dtype == np.float64 and got.shape == (2, 33, 32)
    assert np.array_equal(got, ev.compute_explanations(x, y))           # deterministic per seed
    mel = ev._mel(x.cuda())
    noisy = [ev.method.noisy(mel, s).cpu().numpy() for s in range(3)]
    assert not np.array_equal(noisy[0], noisy[1]) and np.abs(noisy[0] - mel.cpu().numpy()).max() > 0
    assert _rel(got, B.smoothgrad_ref(C.make_model(), mel.cpu().numpy(), y, noisy)) < 1e-4
    ev.method.random_seed = 43
    assert not np.array_equal(got, ev.compute_explanations(x, y))


def test_gradcam_straddling_ties_stable_order(L):
    """n_iter = 7 on the Grad-CAM case: thresholds cut through runs of exact zeros, so the curves depend on
    the tie order. The default (stable) order against the restatement's stable sort, both on the explanation
    the device class computes."""
    case = C.CASES["cam4096"]
    x, y = C.make_inputs(case)
    ev, _ = _evaluator("cam4096", "gradcam")
    expl = ev.compute_explanations(x, y)
    assert any(C.straddling_ties(e, 7) for e in expl)
    cpu = C.make_model()
    for mode in C.MODES:
        scores = getattr(ev, mode)(x, y, 7)
        ref_scores, ref_curves, _ = A.evaluate_auc(cpu, expl, x, y, mode, 7, C.cfg_of(case), sort="stable")
        assert _note("p", np.abs(np.array(ev.insertion_curves) - np.array(ref_curves)).max()) <= 1e-4
        assert _note("score", np.abs(np.array(scores) - np.array(ref_scores)).max()) <= 1e-4


def test_nan_explanation_gives_the_empty_and_the_full_input(L):
    from wam_amd.evalcore import softmax
    case = C.CASES["k4096"]
    x, y = C.make_inputs(case)
    for tie_order in ("stable", "numpy"):
        ev, _ = _evaluator("k4096", "gradcam", tie_order=tie_order)
        ev.explanations = np.full((2, 33, 32), np.nan, dtype=np.float32)
        source = ev._mel(x.cuda())
        with torch.no_grad():
            ends = softmax(ev.model(torch.cat([torch.zeros_like(source), source])).float().cpu().numpy())
        scores = ev.insertion(x, y, 4)
        curves = np.array(ev.insertion_curves)
        assert np.isfinite(curves).all() and np.isfinite(np.array(scores)).all()
        for s in range(2):
            assert abs(curves[s, 0] - ends[s, y[s]]) <= 1e-6 and abs(curves[s, 4] - ends[2 + s, y[s]]) <= 1e-6
