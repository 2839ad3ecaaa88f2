"""wam_waverec2_ranked at the C ABI: the fused plane-resident route bit for bit against the expansion
route, the expansion route bit for bit against the composition the goldens already pin (masks built on
the host as 1.0f / 0.0f, wam_coeff_masks, wam_waverec) and against the float64 oracle, the argument
errors and the Python wrapper.

Bars: bits between the routes and against the composition; the synthesis bar of tests/test_gpu_dwt.py,
4 * 2e-6 * max(1, |ref|max), against oracle.dwt.waverec2 (DESIGN.md section 3.13's bar). Measured on one
MI355X (printed when the module finishes): route 0 against the oracle at most 0.031 of its bar.
"""
import numpy as np
import pytest
import torch

from oracle import dwt

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, 1, 3
I32_MAX = np.iinfo(np.int32).max
WORST = {"dsyn": 0.0}


@pytest.fixture(scope="module")
def L():
    from wam_amd import _lib
    assert torch.cuda.is_available()
    yield _lib
    torch.cuda.synchronize()
    print("[eval2d] worst route 0 synthesis error / bar %.3f" % WORST["dsyn"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def make_case(wavelet, J, shape, C, images, n_iter, deletion, seed=0):
    """Random coefficients (negative values included); per image a random permutation of the cells as
    ranking plus the held slot (rank -1 under insertion, INT32_MAX under deletion); a slot map with
    pad entries (-1), out-of-range entries and held coefficients."""
    from wam_amd.plan import get_plan
    p = get_plan(2, shape, J, wavelet, "symmetric", "cuda")
    K = p.coeff_numel
    rng = np.random.RandomState(seed + 31 * J + n_iter + K)
    coeffs = rng.standard_normal(images * C * K).astype(np.float32)
    assert (coeffs < 0).any()
    cells = K + 3                                                   # more cells than coefficients
    rank = np.stack([rng.permutation(cells) for _ in range(images)]).astype(np.int32)
    rank = np.concatenate([rank, np.full((images, 1), I32_MAX if deletion else -1, np.int32)], 1)
    pos = rng.permutation(cells)[:K].astype(np.int32)
    special = rng.choice(K, 9, replace=False)
    pos[special[:3]] = -1
    pos[special[3:5]] = cells + 6                                   # outside [0, rank_len): reads as -1
    pos[special[5:]] = cells                                        # the held slot
    return p, K, coeffs, rank, pos, int(cells / n_iter)


def ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, deletion, route, out=None, ws=True):
    """wam_waverec2_ranked through the C ABI -> (status, out); the output is prefilled with a sentinel."""
    if out is None:
        out = torch.full((images, n_iter + 1, C) + p.rec_shape, 7.0, device="cuda")
    nb = int(L.lib.wam_waverec2_ranked_workspace_bytes(p.handle, images, C, n_iter, 0))
    assert nb >= int(L.lib.wam_waverec2_ranked_workspace_bytes(p.handle, images, C, n_iter, 1)) > 0
    w = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda") if ws else None
    rc = L.lib.wam_waverec2_ranked(p.handle, images, C, L.ptr(dc), L.ptr(dr), dr.shape[1], L.ptr(dp), n_iter, n_comp,
                                   deletion, route, L.ptr(out), L.ptr(w), L.stream_of(out.device))
    torch.cuda.synchronize()
    return rc, out


def thresholds(n_iter, n_comp, rank_len):
    return [0] + [min(m * n_comp, rank_len) for m in range(1, n_iter)] + [rank_len]


def host_keep(rank_row, pos, n_iter, n_comp, deletion):
    """[n_iter + 1, K] float32 of 1.0 / 0.0: the header's rule on the host."""
    rank_len = rank_row.size
    pad = (pos < 0) | (pos >= rank_len)
    rk = np.where(pad, -1, rank_row[np.where(pad, 0, pos)]).astype(np.int64)
    return np.stack([((rk < t) != bool(deletion)) for t in thresholds(n_iter, n_comp, rank_len)]).astype(np.float32)


def composition(L, p, images, C, coeffs, rank, pos, n_iter, n_comp, deletion):
    """The pinned parts: per image, float masks over the rank slots plus one slot for the pad rule, built
    on the host; wam_coeff_masks; Plan.waverec -> [images, M, C, H, W]."""
    K, M = p.coeff_numel, n_iter + 1
    off = list(p.band_offsets)
    rank_len = rank.shape[1]
    pad = (pos < 0) | (pos >= rank_len)
    dpos = dev(np.where(pad, rank_len, pos).astype(np.int32))
    outs = []
    for n in range(images):
        thr = np.array(thresholds(n_iter, n_comp, rank_len), dtype=np.int64)[:, None]
        slots = np.concatenate([rank[n].astype(np.int64), [-1]])[None, :]             # the pad slot ranks -1
        masks = ((slots < thr) != bool(deletion)).astype(np.float32)
        # the image's planes, band-major over C items
        own = np.concatenate([coeffs[images * C * off[b] + n * C * (off[b + 1] - off[b]):
                                     images * C * off[b] + (n + 1) * C * (off[b + 1] - off[b])]
                              for b in range(p.nbands)])
        masked = torch.empty(M * C * K, dtype=torch.float32, device="cuda")
        dm, do = dev(masks), dev(own)
        assert L.lib.wam_coeff_masks(p.handle, C, L.ptr(do), L.ptr(dpos), M, rank_len + 1, L.ptr(dm), L.ptr(masked),
                                     L.stream_of(masked.device)) == OK
        outs.append(p.waverec(masked, M * C)[0].view((M, C) + p.rec_shape).clone())
    return torch.stack(outs)


FUSED_CASES = {
    # name: (wavelet, J, shape, C, images, n_iter)
    "haar_J1_8x8": ("haar", 1, (8, 8), 1, 1, 4),
    # M = 18: one full and one partial chunk of masks; n_iter does not divide rank_len
    "haar_J3_16x24_n17": ("haar", 3, (16, 24), 3, 1, 17),
    # odd band sizes (11 x 15, 7 x 9) and the crop flag between the levels
    "db2_J2_20x28": ("db2", 2, (20, 28), 3, 1, 6),
    "sym4_J3_40x36": ("sym4", 3, (40, 36), 3, 2, 8),
    "db4_J2_32x32": ("db4", 2, (32, 32), 1, 1, 5),
}


@pytest.mark.parametrize("deletion", [0, 1])
@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_routes_equal_each_other_and_the_pinned_composition_in_bits(L, name, deletion):
    wavelet, J, shape, C, images, n_iter = FUSED_CASES[name]
    p, K, coeffs, rank, pos, n_comp = make_case(wavelet, J, shape, C, images, n_iter, deletion)
    M = n_iter + 1
    if n_iter == 17:
        assert rank.shape[1] % n_iter and M == 18
    if wavelet == "db2":
        assert [s for s in p.band_shapes[:2]] == [(7, 9), (7, 9)] and p.band_shapes[-1] == (11, 15)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    rc1, out1 = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, deletion, 1)
    rc0, out0 = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, deletion, 0)
    assert rc0 == OK and rc1 == OK
    assert not bool((out0 == 7.0).any()) and not bool((out1 == 7.0).any())       # every pixel was written
    assert same_bits(out1, out0), "route 1 vs route 0"
    two_step = composition(L, p, images, C, coeffs, rank, pos, n_iter, n_comp, deletion)
    assert same_bits(out0, two_step), "route 0 vs host masks + wam_coeff_masks + wam_waverec"
    rc, own = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, deletion, -1)
    assert rc == OK and same_bits(own, out0)
    # mask 0 keeps exactly the pad, out-of-range and held entries under insertion, all but the pad and
    # out-of-range ones under deletion (the held slot ranks INT32_MAX there)
    keep = host_keep(rank[0], pos, n_iter, n_comp, deletion)
    assert int(keep[0].sum()) == (K - 5 if deletion else 9)
    # insertion's last mask keeps everything: the plain reconstruction
    if not deletion:
        assert same_bits(out0[:, n_iter], p.waverec(dc, images * C)[0].view((images, C) + p.rec_shape))


def test_misaligned_output_falls_back_to_the_expansion_route(L):
    """An `out` 4 bytes off the 8-byte alignment route 1 states: forcing route 1 is refused and writes
    nothing; the plan's own route still answers, with route 0's bits."""
    wavelet, J, shape, C, images, n_iter = FUSED_CASES["db2_J2_20x28"]
    p, K, coeffs, rank, pos, n_comp = make_case(wavelet, J, shape, C, images, n_iter, 0)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    n = images * (n_iter + 1) * C * p.rec_shape[0] * p.rec_shape[1]
    buf = torch.full((n + 1,), 7.0, device="cuda")
    off = buf[1:].view((images, n_iter + 1, C) + p.rec_shape)
    assert off.data_ptr() % 8 == 4
    rc, _ = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, 0, 1, out=off)
    assert rc == UNSUPPORTED and bool((buf == 7.0).all())
    rc, _ = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, 0, -1, out=off)
    rc0, want = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, 0, 0)
    assert rc == OK and rc0 == OK and same_bits(off, want) and float(buf[0]) == 7.0


def test_python_wrapper_routes(L):
    """Plan.waverec2_ranked on the plan's own route and on both forced ones: the same bits."""
    p, K, coeffs, rank, pos, n_comp = make_case("db2", 2, (20, 28), 3, 2, 5, 1)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    outs = [p.waverec2_ranked(dc, 2, 3, dr, dp, 5, n_comp, True, route=r) for r in (-1, 0, 1)]
    assert outs[0].shape == (2, 6, 3, 20, 28) and same_bits(outs[0], outs[1]) and same_bits(outs[1], outs[2])
    assert p.ranked2_route() in (0, 1)
    with pytest.raises(TypeError):
        p.waverec2_ranked(dc, 2, 3, dr.long(), dp, 5, n_comp, True)
    with pytest.raises(ValueError):
        p.waverec2_ranked(dc, 1, 3, dr, dp, 5, n_comp, True)


ORACLE_CASES = {
    "haar_J3_16x24": ("haar", 3, (16, 24)),
    "db2_J2_20x28": ("db2", 2, (20, 28)),
    "db6_J2_24x24": ("db6", 2, (24, 24)),        # 12 taps: beyond the plane-resident synthesis
}


@pytest.mark.parametrize("deletion", [0, 1])
@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_expansion_route_against_the_oracle(L, name, deletion):
    wavelet, J, shape = ORACLE_CASES[name]
    images, C, n_iter = 2, 3, 3
    p, K, coeffs, rank, pos, n_comp = make_case(wavelet, J, shape, C, images, n_iter, deletion, seed=5)
    M = n_iter + 1
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    if wavelet == "db6":
        assert p.ranked2_route() == 0
        rc, sentinel = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, deletion, 1)
        assert rc == UNSUPPORTED and bool((sentinel == 7.0).all())
    rc, out = ranked(L, p, images, C, dc, dr, dp, n_iter, n_comp, deletion, 0)
    assert rc == OK
    got = out.cpu().numpy()
    off = list(p.band_offsets)
    planes = images * C
    for n in range(images):
        keep = host_keep(rank[n], pos, n_iter, n_comp, deletion).astype(np.float64)
        for c in range(C):
            i = n * C + c
            flat = np.concatenate([coeffs[planes * off[b] + i * (off[b + 1] - off[b]):
                                          planes * off[b] + (i + 1) * (off[b + 1] - off[b])]
                                   for b in range(p.nbands)]).astype(np.float64)
            for m in range(M):
                v = flat * keep[m]
                bands = [v[off[b]:off[b + 1]].reshape(p.band_shapes[b]) for b in range(p.nbands)]
                ref = dwt.waverec2([bands[0]] + [tuple(bands[1 + 3 * l:4 + 3 * l]) for l in range(J)], wavelet)
                bar = 4 * 2e-6 * max(1.0, float(np.abs(ref).max()))
                err = float(np.abs(got[n, m, c] - ref).max())
                WORST["dsyn"] = max(WORST["dsyn"], err / bar)
                assert err <= bar, (name, n, m, c, err, bar)


def test_argument_errors_launch_nothing(L):
    from wam_amd.plan import get_plan
    p, K, coeffs, rank, pos, n_comp = make_case("haar", 1, (8, 8), 1, 1, 4, 0)
    dc, dr, dp = dev(coeffs), dev(rank), dev(pos)
    out = torch.full((1, 5, 1, 8, 8), 7.0, device="cuda")
    w = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    st = L.stream_of(out.device)
    rl = rank.shape[1]

    def call(plan=p, images=1, channels=1, c=dc, r=dr, rank_len=rl, ps=dp, n_iter=4, n_comp=4, route=-1, o=out, ws=w):
        return L.lib.wam_waverec2_ranked(plan.handle if plan is not None else None, images, channels, L.ptr(c), L.ptr(r),
                                         rank_len, L.ptr(ps), n_iter, n_comp, 0, route, L.ptr(o), L.ptr(ws), st)

    p3 = get_plan(3, (8, 8, 8), 1, "haar", "symmetric", "cuda")
    p12 = get_plan(2, (24, 24), 1, "db6", "symmetric", "cuda")
    assert call(plan=p3) == UNSUPPORTED
    assert call(plan=p12, route=1) == UNSUPPORTED
    assert call(plan=None) == INVALID
    for kw in ({"c": None}, {"r": None}, {"ps": None}, {"o": None}, {"images": -1}, {"channels": 0}, {"channels": 5},
               {"rank_len": 0}, {"rank_len": 1 << 31}, {"n_iter": 0}, {"n_comp": -1}, {"route": 2}, {"route": -2},
               {"ws": None, "route": 0}, {"ws": w[4:], "route": 0}, {"ws": None, "route": 1},
               {"n_iter": 65535 * 16 + 1, "route": 0}):
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                             # nothing was launched
    assert call(images=0, ws=None) == OK                                        # no images: nothing to do
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert L.lib.wam_waverec2_ranked_route(p.handle) in (0, 1)
    assert L.lib.wam_waverec2_ranked_route(p3.handle) < 0
    assert L.lib.wam_waverec2_ranked_workspace_bytes(p3.handle, 1, 1, 4, 0) == 0
