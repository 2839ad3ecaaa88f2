"""wam_waverec1_ranked and wam_peak_divide at the C ABI, written from the contract sentences of
include/wam_hip.h: the two routes against each other and against the composition they replace
(tests/eval1d_ref.rank_mask_coeffs_ref + Plan.waverec) in bits, row_max against the rows' own maxima in
bits, route 0 against the float64 oracle within the synthesis bar of tests/test_gpu_dwt.py, the plans
route 1 does not serve, the argument checks, and wam_peak_divide against wam_peak_normalize in bits.

Measured on one MI355X: worst |route 0 - oracle| / bar = 0.025 (printed by test_route0_against_the_oracle).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval1d_ref as R

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, 1, 3
SENT = 7.0
GUARD = 64

# wavelet, J, n, sets, n_iter: the smallest geometries at which the fused kernel can go wrong
GEOMS = {
    "haar_J1_n8": ("haar", 1, 8, 2, 3),
    "haar_J3_n64_M18": ("haar", 3, 64, 2, 17),      # M = 18: a partial chunk of masks, n_iter does not divide K
    "db2_J2_n37": ("db2", 2, 37, 2, 5),             # odd bands, reconstruction 38 long
    "db6_J5_n8200": ("db6", 5, 8200, 2, 4),         # two tiles, the last with 8 outputs: clamped ranges
    "sym4_J4_n20001": ("sym4", 4, 20001, 3, 4),     # three tiles, odd length
    "db10_J2_n9000": ("db10", 2, 9000, 1, 4),       # 20 taps
}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def make_case(plan, sets, n_iter, seed):
    """Random coefficients (negative values included), a random permutation as ranking over rank_len =
    K - 3 slots, and a slot map with shared slots, -1 entries and out-of-range entries."""
    rng = np.random.RandomState(seed)
    K = plan.coeff_numel
    rank_len = max(1, K - 3)
    coeffs = rng.standard_normal(sets * K).astype(np.float32)
    rank = np.stack([rng.permutation(rank_len) for _ in range(sets)]).astype(np.int32)
    pos = rng.randint(0, rank_len, K).astype(np.int32)      # drawn with replacement: duplicated slots
    pos[rng.choice(K, max(1, K // 9), replace=False)] = -1
    pos[rng.choice(K, max(1, K // 11), replace=False)] = rank_len + 5
    pos[K // 2] = np.iinfo(np.int32).min
    return coeffs, rank, pos, rank_len, int(rank_len / n_iter)


def composition(plan, sets, coeffs, rank, pos, n_iter, n_comp, deletion):
    """The reference: the contract's mask expansion in numpy, then the plan's own wam_waverec."""
    masked = R.rank_mask_coeffs_ref(list(plan.band_offsets), sets, coeffs, rank, pos, n_iter, n_comp, deletion)
    return masked, plan.waverec(dev(masked), sets * (n_iter + 1))[0].view(sets * (n_iter + 1), -1)


def call(L, plan, sets, dc, dr, rank_len, dp, n_iter, n_comp, deletion, route, want_max=True, offset=0):
    """-> (status, out [rows, rec_len] view, row_max or None, the whole buffer): out starts `offset`
    floats into a sentinel-filled buffer that ends in a guard."""
    rows, rec_len = sets * (n_iter + 1), plan.rec_shape[0]
    buf = torch.full((offset + rows * rec_len + GUARD,), SENT, device="cuda")
    out = buf[offset:offset + rows * rec_len]
    row_max = torch.full((rows + 4,), SENT, device="cuda") if want_max else None
    n = int(L.lib.wam_waverec1_ranked_workspace_bytes(plan.handle, sets, n_iter, route))
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda")
    rc = L.lib.wam_waverec1_ranked(plan.handle, sets, L.ptr(dc), L.ptr(dr), rank_len, L.ptr(dp), n_iter, n_comp,
                                   deletion, route, L.ptr(out), L.ptr(row_max), L.ptr(ws), L.stream_of(buf.device))
    torch.cuda.synchronize()
    return rc, out.view(rows, rec_len), row_max, buf


def guard_intact(buf, offset, used):
    return bool((buf[:offset] == SENT).all()) and bool((buf[offset + used:] == SENT).all())


@pytest.mark.parametrize("deletion", [0, 1])
@pytest.mark.parametrize("name", list(GEOMS))
def test_routes_agree_with_the_composition_in_bits(L, name, deletion):
    """Route 1 = route 0 = rank_mask_coeffs_ref + Plan.waverec in bits; row_max = the rows' own maxima
    in bits on both routes; deletion's last row drops everything: zeros and a +0.0f maximum; a NULL
    row_max works; nothing is written past the output."""
    from wam_amd.plan import get_plan
    wavelet, J, n, sets, n_iter = GEOMS[name]
    plan = get_plan(1, (n,), J, wavelet, "reflect", "cuda")
    coeffs, rank, pos, rank_len, n_comp = make_case(plan, sets, n_iter, n + deletion)
    _, ref = composition(plan, sets, coeffs, rank, pos, n_iter, n_comp, deletion)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    rows, rec_len = sets * (n_iter + 1), plan.rec_shape[0]
    assert rec_len == n + n % 2
    for route in (0, 1):
        rc, out, row_max, buf = call(L, plan, sets, dc, dr, rank_len, dp, n_iter, n_comp, deletion, route)
        assert rc == OK, (name, route, rc)
        assert guard_intact(buf, 0, rows * rec_len) and bool((row_max[rows:] == SENT).all())
        assert np.array_equal(bits(out), bits(ref)), "%s route %d: out differs from the composition" % (name, route)
        assert np.array_equal(bits(row_max[:rows]), bits(out.amax(dim=1))), "%s route %d: row_max" % (name, route)
        if deletion:
            last = np.arange(sets) * (n_iter + 1) + n_iter
            assert not bits(out)[last].any() and not bits(row_max[:rows])[last].any()      # +0.0f, not -0.0f
        rc, out2, none, buf = call(L, plan, sets, dc, dr, rank_len, dp, n_iter, n_comp, deletion, route, want_max=False)
        assert rc == OK and none is None and np.array_equal(bits(out2), bits(ref))
        assert guard_intact(buf, 0, rows * rec_len)


@pytest.mark.parametrize("name", ["haar_J3_n64_M18", "db2_J2_n37", "db6_J5_n8200"])
def test_route0_against_the_oracle(L, name):
    """Route 0 vs oracle.dwt.waverec of the masked float64 coefficients, within the synthesis bar of
    tests/test_gpu_dwt.py over the J levels' worth of roundings: 4 * 2e-6 * max(1, |ref|max)."""
    from oracle import dwt
    from wam_amd.plan import get_plan
    wavelet, J, n, sets, n_iter = GEOMS[name]
    plan = get_plan(1, (n,), J, wavelet, "reflect", "cuda")
    coeffs, rank, pos, rank_len, n_comp = make_case(plan, sets, n_iter, n)
    off = list(plan.band_offsets)
    rows = sets * (n_iter + 1)
    masked = R.rank_mask_coeffs_ref(off, sets, coeffs, rank, pos, n_iter, n_comp, 0).astype(np.float64)
    bands = [masked[rows * off[b]:rows * off[b + 1]].reshape(rows, -1) for b in range(len(off) - 1)]
    ref = dwt.waverec(bands, wavelet)
    rc, out, _, _ = call(L, plan, sets, dev(coeffs), dev(rank), rank_len, dev(pos), n_iter, n_comp, 0, 0)
    assert rc == OK and ref.shape == tuple(out.shape)
    bar = 4 * 2e-6 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print("[eval1d_ranked] %s: |route 0 - oracle| = %.3e, bar %.3e, ratio %.3f" % (name, err, bar, err / bar))
    assert err <= bar


@pytest.mark.parametrize("what", ["J9", "generic", "periodic"])
def test_plans_route1_does_not_serve(L, what):
    """The route query says 0, forcing route 1 returns WAM_ERR_UNSUPPORTED with the output untouched,
    the plan's own route computes the composition's bits."""
    from wam_amd.plan import get_plan
    if what == "J9":
        plan, n_iter = get_plan(1, (8192,), 9, "haar", "reflect", "cuda"), 4
    elif what == "generic":
        plan, n_iter = get_plan(1, (64,), 3, "haar", "reflect", "cuda", generic=True), 4
    else:
        plan, n_iter = get_plan(1, (64,), 3, "haar", "periodic", "cuda"), 4
    sets = 2
    assert plan.ranked1_route() == 0
    coeffs, rank, pos, rank_len, n_comp = make_case(plan, sets, n_iter, 5)
    _, ref = composition(plan, sets, coeffs, rank, pos, n_iter, n_comp, 0)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    rc, out, row_max, buf = call(L, plan, sets, dc, dr, rank_len, dp, n_iter, n_comp, 0, 1)
    assert rc == UNSUPPORTED and bool((buf == SENT).all()) and bool((row_max == SENT).all())
    rc, out, row_max, buf = call(L, plan, sets, dc, dr, rank_len, dp, n_iter, n_comp, 0, -1)
    assert rc == OK and np.array_equal(bits(out), bits(ref))
    assert np.array_equal(bits(row_max[:out.shape[0]]), bits(out.amax(dim=1)))


def test_non_1d_plans_and_invalid_arguments(L):
    from wam_amd.plan import get_plan
    lib = L.lib
    st = L.stream_of(torch.device("cuda"))
    buf = torch.zeros(4096, device="cuda")
    p = L.ptr(buf)
    for plan in (get_plan(2, (16, 16), 1, "haar", "symmetric", "cuda"), get_plan(3, (8, 8, 8), 1, "haar", "symmetric", "cuda")):
        assert lib.wam_waverec1_ranked_route(plan.handle) == -UNSUPPORTED
        assert lib.wam_waverec1_ranked_workspace_bytes(plan.handle, 1, 4, 0) == 0
        assert lib.wam_waverec1_ranked(plan.handle, 1, p, p, 8, p, 4, 2, 0, -1, p, p, p, st) == UNSUPPORTED
    plan = get_plan(1, (64,), 3, "haar", "reflect", "cuda")
    h = plan.handle
    good = dict(plan=h, sets=1, coeffs=p, rank=p, rank_len=64, pos=p, n_iter=4, n_comp=16, deletion=0, route=-1,
                out=p, row_max=p, ws=p, stream=st)
    bad = [dict(plan=None), dict(sets=-1), dict(coeffs=None), dict(rank=None), dict(rank_len=0),
           dict(rank_len=2 ** 31), dict(pos=None), dict(n_iter=0), dict(n_comp=-1), dict(route=2), dict(route=-2),
           dict(out=None), dict(ws=None), dict(ws=ctypes.c_void_p(buf.data_ptr() + 4)),
           dict(n_iter=65535 * 16)]                      # 65535 * 16 + 1 masks
    for change in bad:
        a = dict(good, **change)
        assert lib.wam_waverec1_ranked(*a.values()) == INVALID, change
    assert not buf.any()                                  # nothing was launched
    assert lib.wam_waverec1_ranked(*dict(good, sets=0, ws=None).values()) == OK
    for args in ((None, 1, 4, 0), (h, -1, 4, 0), (h, 1, 0, 0), (h, 1, 4, 2), (h, 1, 4, -2)):
        assert lib.wam_waverec1_ranked_workspace_bytes(*args) == 0
    K, M = plan.coeff_numel, 5
    b0 = lib.wam_waverec1_ranked_workspace_bytes(h, 3, 4, 0)
    assert b0 == (3 * M * K * 4 + 15) // 16 * 16 + lib.wam_plan_workspace_bytes(h, 3 * M)
    assert lib.wam_waverec1_ranked_workspace_bytes(h, 3, 4, 1) == (3 * K * 4 + 15) // 16 * 16
    assert lib.wam_waverec1_ranked_workspace_bytes(h, 3, 4, -1) == b0
    assert lib.wam_waverec1_ranked_route(None) == -INVALID
    # wam_peak_divide's own list
    ok = dict(rows=2, len=8, inp=p, row_max=p, out=p, silent=None, zero_silent=0, stream=st)
    for change in (dict(rows=-1), dict(rows=2 ** 31), dict(len=0), dict(inp=None), dict(row_max=None), dict(out=None)):
        assert lib.wam_peak_divide(*dict(ok, **change).values()) == INVALID, change
    assert lib.wam_peak_divide(*dict(ok, rows=0).values()) == OK


@pytest.mark.parametrize("name", ["db2_J2_n37", "db6_J5_n8200"])
def test_output_four_bytes_off(L, name):
    """An `out` 4 bytes off 16-byte alignment: forced route 1 either serves it with the right bits or
    refuses and writes nothing; the plan's own route serves it."""
    from wam_amd.plan import get_plan
    wavelet, J, n, sets, n_iter = GEOMS[name]
    plan = get_plan(1, (n,), J, wavelet, "reflect", "cuda")
    coeffs, rank, pos, rank_len, n_comp = make_case(plan, sets, n_iter, n)
    _, ref = composition(plan, sets, coeffs, rank, pos, n_iter, n_comp, 1)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    rows, rec_len = sets * (n_iter + 1), plan.rec_shape[0]
    rc, out, row_max, buf = call(L, plan, sets, dc, dr, rank_len, dp, n_iter, n_comp, 1, 1, offset=1)
    assert out.data_ptr() % 8 == 4
    if rc == UNSUPPORTED:
        assert bool((buf == SENT).all())
    else:
        assert rc == OK and np.array_equal(bits(out), bits(ref)) and guard_intact(buf, 1, rows * rec_len)
        assert np.array_equal(bits(row_max[:rows]), bits(out.amax(dim=1)))
    rc, out, row_max, buf = call(L, plan, sets, dc, dr, rank_len, dp, n_iter, n_comp, 1, -1, offset=1)
    assert rc == OK and np.array_equal(bits(out), bits(ref)) and guard_intact(buf, 1, rows * rec_len)
    assert np.array_equal(bits(row_max[:rows]), bits(out.amax(dim=1)))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099, 20002])
def test_peak_divide(L, n, in_place):
    """wam_peak_divide with numpy's maxima vs peak_normalize_ref and vs wam_peak_normalize's own output,
    in bits, on the 7-row pattern of test_peak_normalize (maximum first, maximum last, all negative, all
    zero, non-positive with zeros, random); the silent flags equal. 64 and 20,002's aligned rows take the
    16-byte path; 4,099 and 20,002 span more than one workgroup per row."""
    rng = np.random.RandomState(n)
    x = rng.uniform(-1, 1, (7, n)).astype(np.float32)
    x[0, 0], x[1, -1] = 3.0, 2.5
    x[2] = -np.abs(x[2]) - 0.25
    x[3] = 0.0
    x[4] = -np.abs(x[4])
    x[4, n // 2] = 0.0
    mx = dev(x.max(axis=1))
    for zero_silent in (0, 1):
        src = dev(x)
        out = src if in_place else torch.full_like(src, SENT)
        silent = torch.full((7,), -1, dtype=torch.int32, device="cuda")
        L.check(L.lib.wam_peak_divide(7, n, L.ptr(src), L.ptr(mx), L.ptr(out), L.ptr(silent), zero_silent,
                                      L.stream_of(src.device)))
        ref, ref_silent = R.peak_normalize_ref(x, zero_silent)
        assert silent.cpu().tolist() == ref_silent.tolist() == [0, 0, 0, 1, 1, 0, 0]
        R.assert_bits(out.cpu().numpy(), ref, "peak_divide n=%d zero_silent=%d in_place=%d" % (n, zero_silent, in_place))
        src2 = dev(x)
        norm, silent2 = torch.full_like(src2, SENT), torch.full((7,), -1, dtype=torch.int32, device="cuda")
        L.check(L.lib.wam_peak_normalize(7, n, L.ptr(src2), L.ptr(norm), L.ptr(silent2), zero_silent,
                                         L.stream_of(src2.device)))
        R.assert_bits(out.cpu().numpy(), norm.cpu().numpy(), "peak_divide vs peak_normalize n=%d" % n)
        assert torch.equal(silent, silent2)
        if not in_place:
            assert torch.equal(src, dev(x))
        L.check(L.lib.wam_peak_divide(7, n, L.ptr(src2), L.ptr(mx), L.ptr(norm), None, zero_silent,
                                      L.stream_of(src2.device)))          # a NULL silent
