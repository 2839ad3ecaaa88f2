"""Eval3DWAM on the device: wam_waverec_ranked at the C ABI -- the fused 3D Haar route bit for bit against
the expansion route and against the two-step route the test builds itself (rank_mask_coeffs_ref of
tests/eval1d_ref.py, then Plan.waverec), the expansion route alone against the float64 oracle where the
fused kernel does not apply -- and the class against the float64 restatement of tests/eval3d_ref.py.

Bars: bits between the routes; the synthesis bar of tests/test_gpu_dwt.py, 4 * 2e-6 * max(1, |ref|max),
against oracle.dwt.waverec3; R.BAR = 1e-4 absolute on class probabilities (the 2D evaluator's bar,
tests/eval1d_ref.py) for curves, scores and faithfulness, as tests/test_gpu_eval1d.py holds them.
Measured on one MI355X (printed when the module finishes): worst |p(device) - p(restatement)| 1.19e-7,
worst score error 1.79e-7, worst faithfulness error 5.96e-8; route 0 against the oracle at most 0.024 of
its bar.
"""
import numpy as np
import pytest
import torch

from oracle import dwt
from tests import eval1d_ref as R1
from tests import eval3d_ref as R

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, 1, 3
WORST = {"dp": 0.0, "dscore": 0.0, "dff": 0.0, "dsyn": 0.0}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()
    print("[eval3d] worst |device - restatement|: p %.3e, score %.3e, faithfulness %.3e (bar %.1e); worst route 0 "
          "synthesis error / bar %.3f" % (WORST["dp"], WORST["dscore"], WORST["dff"], R.BAR, WORST["dsyn"]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_case(shape, J, sets, n_iter, wavelet="haar", seed=0, out_of_range=False):
    """Random coefficients (negative values included), ranks that are random permutations (no ties) and
    a slot map that is a random permutation with a few pad entries."""
    from wam_amd.plan import get_plan
    p = get_plan(3, shape, J, wavelet, "symmetric", "cuda")
    K = p.coeff_numel
    rng = np.random.RandomState(seed + 17 * J + n_iter)
    coeffs = rng.standard_normal(sets * K).astype(np.float32)
    assert (coeffs < 0).any()
    rank = np.stack([rng.permutation(K) for _ in range(sets)]).astype(np.int32)
    pos = rng.permutation(K).astype(np.int32)
    pos[rng.choice(K, 5, replace=False)] = -1
    if out_of_range:
        pos[rng.choice(K, 2, replace=False)] = K + 5
    return p, K, coeffs, rank, pos


def ranked(L, p, sets, dc, dr, dp, K, n_iter, deletion, route, out=None, ws=True):
    """wam_waverec_ranked through the C ABI -> (status, out); the output is prefilled with a sentinel."""
    M = n_iter + 1
    if out is None:
        out = torch.full((sets * M,) + p.rec_shape, 7.0, device="cuda")
    nb = int(L.lib.wam_waverec_ranked_workspace_bytes(p.handle, sets, n_iter, 0))
    w = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda") if ws else None
    rc = L.lib.wam_waverec_ranked(p.handle, sets, L.ptr(dc), L.ptr(dr), K, L.ptr(dp), n_iter, int(K / n_iter), deletion,
                                  route, L.ptr(out), L.ptr(w), L.stream_of(out.device))
    torch.cuda.synchronize()
    return rc, out


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


FUSED_CASES = {
    # fewer blocks than a wave
    "8x8x8_J1": ((8, 8, 8), 1, 1, 4, (0,)),
    # M = 18: one full and one partial mask chunk; n_iter does not divide K: the forced-full last mask;
    # cross-item offsets
    "8x8x8_J2_n17": ((8, 8, 8), 2, 3, 17, (1,)),
    # non-cubic strides
    "8x12x16_J2": ((8, 12, 16), 2, 2, 5, (0, 1)),
    # several rows of blocks, five mask chunks
    "16x16x16_J2_n64": ((16, 16, 16), 2, 2, 64, (0, 1)),
}


@pytest.mark.parametrize("name,deletion", [(n, d) for n, c in FUSED_CASES.items() for d in c[4]])
def test_fused_route_equals_expansion_route_in_bits(L, name, deletion):
    shape, J, sets, n_iter, _ = FUSED_CASES[name]
    p, K, coeffs, rank, pos = make_case(shape, J, sets, n_iter, out_of_range=name == "8x12x16_J2")
    M = n_iter + 1
    if name == "8x8x8_J2_n17":
        assert int(K / n_iter) * n_iter < K and M == 18
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    rc1, out1 = ranked(L, p, sets, dc, dr, dp, K, n_iter, deletion, 1, ws=False)   # route 1 reads no workspace
    rc0, out0 = ranked(L, p, sets, dc, dr, dp, K, n_iter, deletion, 0)
    assert rc0 == OK and rc1 == OK
    masked = R1.rank_mask_coeffs_ref(list(p.band_offsets), sets, coeffs, rank, pos, n_iter, int(K / n_iter), deletion)
    two_step = p.waverec(dev(masked), sets * M)[0]
    assert not bool((out0 == 7.0).any()) and not bool((out1 == 7.0).any())     # every voxel was written
    assert same_bits(out0, two_step), "route 0 vs rank_mask_coeffs_ref + waverec"
    assert same_bits(out1, two_step), "route 1 vs rank_mask_coeffs_ref + waverec"
    assert same_bits(out1, out0)
    # the plan's own route gives the same volumes, whichever it is
    rc, own = ranked(L, p, sets, dc, dr, dp, K, n_iter, deletion, -1)
    assert rc == OK and same_bits(own, two_step)
    # insertion's last mask keeps everything, the pad slots included: the plain reconstruction
    if not deletion:
        assert same_bits(out1.view((sets, M) + p.rec_shape)[:, n_iter], p.waverec(dc, sets)[0])


def test_python_wrapper_routes(L):
    """Plan.waverec_ranked on the plan's own route and on both forced ones: the same bits."""
    p, K, coeffs, rank, pos = make_case((8, 8, 8), 2, 2, 5)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    outs = [p.waverec_ranked(dc, 2, dr, dp, 5, int(K / 5), True, route=r) for r in (-1, 0, 1)]
    assert outs[0].shape == (12, 8, 8, 8) and same_bits(outs[0], outs[1]) and same_bits(outs[1], outs[2])
    assert p.ranked_route in (0, 1)


ROUTE0_CASES = {
    "haar_J3_16": ((16, 16, 16), 3, "haar"),
    "haar_J2_10": ((10, 10, 10), 2, "haar"),      # not divisible by 4
    "db2_J2_12": ((12, 12, 12), 2, "db2"),
}


@pytest.mark.parametrize("deletion", [0, 1])
@pytest.mark.parametrize("name", list(ROUTE0_CASES))
def test_expansion_route_against_the_oracle(L, name, deletion):
    shape, J, wavelet = ROUTE0_CASES[name]
    sets, n_iter = 2, 3
    p, K, coeffs, rank, pos = make_case(shape, J, sets, n_iter, wavelet=wavelet, seed=5)
    M = n_iter + 1
    assert p.ranked_route == 0
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    rc, sentinel = ranked(L, p, sets, dc, dr, dp, K, n_iter, deletion, 1)
    assert rc == UNSUPPORTED and bool((sentinel == 7.0).all())
    rc, out = ranked(L, p, sets, dc, dr, dp, K, n_iter, deletion, 0)
    assert rc == OK
    rc, own = ranked(L, p, sets, dc, dr, dp, K, n_iter, deletion, -1)
    assert rc == OK and same_bits(own, out)
    off = list(p.band_offsets)
    masked = R1.rank_mask_coeffs_ref(off, sets, coeffs, rank, pos, n_iter, int(K / n_iter), deletion).astype(np.float64)
    got = out.cpu().numpy()
    assert got.shape == (sets * M,) + p.rec_shape
    for i in range(sets * M):
        bands = [masked[sets * M * off[b] + i * (off[b + 1] - off[b]):sets * M * off[b] + (i + 1) * (off[b + 1] - off[b])]
                 .reshape(p.band_shapes[b]) for b in range(p.nbands)]
        cont = [bands[0]] + [dict(zip(R.KEYS3, bands[1 + 7 * l:8 + 7 * l])) for l in range(J)]
        ref = dwt.waverec3(cont, wavelet)
        bar = 4 * 2e-6 * max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(got[i] - ref).max())
        WORST["dsyn"] = max(WORST["dsyn"], err / bar)
        assert err <= bar, (name, i, err, bar)


def test_argument_errors(L):
    from wam_amd.plan import get_plan
    p, K, coeffs, rank, pos = make_case((8, 8, 8), 1, 1, 4)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    out = torch.full((5, 8, 8, 8), 7.0, device="cuda")
    w = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    st = L.stream_of(out.device)
    call = lambda plan, n_iter, o, route=-1: L.lib.wam_waverec_ranked(  # noqa: E731
        plan.handle, 1, L.ptr(dc), L.ptr(dr), K, L.ptr(dp), n_iter, 4, 0, route, L.ptr(o), L.ptr(w), st)
    p2 = get_plan(2, (16, 32), 1, "haar", "symmetric", "cuda")
    assert call(p2, 4, out) == UNSUPPORTED
    assert call(p, 0, out) == INVALID
    assert call(p, 4, None) == INVALID
    assert call(p, 4, out, route=2) == INVALID
    assert L.lib.wam_waverec_ranked(p.handle, 1, L.ptr(dc), L.ptr(dr), K, L.ptr(dp), 4, 4, 0, 0, L.ptr(out), None,
                                    st) == INVALID                              # route 0 without a workspace
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                             # nothing was launched
    assert L.lib.wam_waverec_ranked(p.handle, 0, L.ptr(dc), L.ptr(dr), K, L.ptr(dp), 4, 4, 0, -1, L.ptr(out), None,
                                    st) == OK                                   # no sets: nothing to do
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------ the class
CLASS_CASES = {"J1_8": (8, 1), "J2_8": (8, 2), "J3_16": (16, 3)}     # J <= 2: the fused route; J = 3: route 0
Y = [1, 3, 7]
N_ITER = 8
_EVALS = {}


def volumes(S):
    return torch.rand(3, 1, S, S, S, generator=torch.Generator().manual_seed(S))


def make_eval(name, **kw):
    import testmodels
    from wam_amd.evaluation import Eval3DWAM
    S, J = CLASS_CASES[name]
    return Eval3DWAM(testmodels.TinyVoxel().cuda(), wavelet="haar", J=J, n_samples=2, **kw)


def shared_eval(name):
    """One evaluator per case, its grad_wams computed by the first test that needs them."""
    if name not in _EVALS:
        ev = make_eval(name)
        calls = []
        inner = ev.gradwam
        ev.gradwam = lambda *a: calls.append(1) or inner(*a)
        _EVALS[name] = (ev, calls)
    return _EVALS[name]


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    d = float(np.abs(got - want).max())
    print("[eval3d] %s: max |d| = %.3e" % (what, d))
    return d


@pytest.mark.parametrize("name", list(CLASS_CASES))
def test_class_against_the_restatement(L, name):
    """insertion, deletion, faithfulness and input fidelity against tests/eval3d_ref.py fed the
    evaluator's own grad_wams; grad_wams are computed once."""
    import testmodels
    from wam_amd.plan import get_plan
    S, J = CLASS_CASES[name]
    x = volumes(S)
    ev, calls = shared_eval(name)
    if J == 3:
        assert get_plan(3, (S, S, S), J, "haar", "symmetric", "cuda").ranked_route == 0
    model = testmodels.TinyVoxel()
    for mode in ("insertion", "deletion"):
        scores = getattr(ev, mode)(x, Y, n_iter=N_ITER)
        curves = getattr(ev, mode + "_curves")
        assert len(calls) == 1                                   # the second call does not recompute grad_wams
        gw = ev.grad_wams
        assert gw.shape == (3, S, S, S)
        want_scores, want_curves, _ = R.evaluate_auc(model, x.numpy(), Y, gw, mode, N_ITER, J)
        assert np.array(curves).shape == (3, N_ITER + 1)
        dp = close(curves, want_curves, "%s %s curves" % (name, mode))
        ds = close(scores, want_scores, "%s %s scores" % (name, mode))
        WORST["dp"], WORST["dscore"] = max(WORST["dp"], dp), max(WORST["dscore"], ds)
        assert dp <= R.BAR and ds <= R.BAR, (name, mode, dp, ds)
    dff = close(ev.faithfulness(x, Y), R.faithfulness(model, x.numpy(), Y, ev.grad_wams, J), name + " faithfulness")
    WORST["dff"] = max(WORST["dff"], dff)
    assert dff <= R.BAR
    assert ev.input_fidelity(x, Y) == R.input_fidelity(model, x.numpy(), Y, ev.grad_wams, J)
    assert len(calls) == 1 and isinstance(scores, list)
    # the ends of the paths: the full volume is what the model sees without masking
    with torch.no_grad():
        base = R.softmax(testmodels.TinyVoxel().cuda()(x.cuda()).cpu().numpy())
    for i in range(3):
        assert abs(ev.insertion_curves[i][-1] - base[i, Y[i]]) <= R.BAR
        assert abs(ev.deletion_curves[i][0] - base[i, Y[i]]) <= R.BAR


@pytest.mark.parametrize("name", ["J2_8", "J3_16"])
def test_eval_batch_does_not_change_the_curves(L, name):
    """eval_batch = n_iter + 1 (one volume per forward) and the default (all three in one)."""
    S, J = CLASS_CASES[name]
    x = volumes(S)
    ev, _ = shared_eval(name)
    if ev.grad_wams is None:
        ev.insertion(x, Y, n_iter=N_ITER)
    one = make_eval(name, eval_batch=N_ITER + 1)
    one.grad_wams = ev.grad_wams
    for mode in ("insertion", "deletion"):
        getattr(one, mode)(x, Y, n_iter=N_ITER), getattr(ev, mode)(x, Y, n_iter=N_ITER)
        assert close(getattr(one, mode + "_curves"), getattr(ev, mode + "_curves"), "eval_batch %s %s" % (name, mode)) <= R.BAR


def test_y_none_and_bad_volumes_raise(L):
    ev = make_eval("J2_8")
    with pytest.raises(ValueError, match="labels"):
        ev.insertion(volumes(8), None)
    ev.grad_wams = np.zeros((1, 10, 10, 10), np.float32)
    with pytest.raises(ValueError, match="bijection onto the coefficients"):
        ev.insertion(torch.rand(1, 1, 10, 10, 10), [0], n_iter=4)
    ev.grad_wams = np.zeros((1, 8, 8, 16), np.float32)
    with pytest.raises(ValueError, match="cubic"):
        ev.insertion(torch.rand(1, 1, 8, 8, 16), [0], n_iter=4)
