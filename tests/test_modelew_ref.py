"""The numpy references of tests/modelew_ref.py pinned to torch on the CPU: the elementwise
references (fp32 and bf16) against torch.relu / adds / .to(bfloat16) / torch.where, the max pool
against F.max_pool2d(return_indices=True) and aten.max_pool2d_with_indices_backward over the
geometry list, and the tie / -inf / NaN rules on hand-built planes. No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import modelew_ref as R

F32 = np.float32
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127     # + 2^119 is (2 - 2^-8) 2^127: finite in fp32, the tie to infinity in bf16
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, BF16_MAX, 2.0 ** 119, 1.0, 1.0078125, 2.0 ** -8,
                     -1.0, -1.0078125, -2.0 ** -8], dtype=F32)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32))


def bits_of(t):
    """torch bf16 tensor -> uint16 patterns"""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def bf16_values(rng, n):
    """n float32 values that are exact in bf16"""
    return R.store(rng.standard_normal(n).astype(F32) * F32(2.0), True)


# ------------------------------------------------------------------------------ bf16 helpers
def test_bf16_helpers_match_torch():
    """Every one of the 65,536 patterns widens as torch widens it; rounding agrees with torch on
    random values, on every tie of a short range in both directions, on overflow to infinity and
    keeps NaN a NaN."""
    allbits = np.arange(65536, dtype=np.uint16)
    wide = R.bf16_to_f32(allbits)
    tw = torch.from_numpy(allbits.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.array_equal(wide.view(np.uint32), tw.view(np.uint32))
    back = R.f32_to_bf16(wide)
    nan = np.isnan(wide)
    assert np.array_equal(back[~nan], allbits[~nan]) and np.isnan(R.bf16_to_f32(back[nan])).all()
    rng = np.random.RandomState(0)
    v = (rng.standard_normal(20000) * 10.0 ** rng.uniform(-30, 30, 20000)).astype(F32)
    # ties: a bf16 value plus half of its spacing, for even and odd last bits
    base = R.bf16_to_f32(np.arange(0x3f80, 0x3fa0, dtype=np.uint16))
    ties = (base.view(np.uint32) | np.uint32(0x8000)).view(F32)
    big = np.array([BF16_MAX, BF16_MAX + 2.0 ** 119, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, 0.0, -0.0], dtype=F32)
    v = np.concatenate([v, ties, -ties, big])
    assert np.array_equal(R.f32_to_bf16(v), bits_of(t32(v).to(torch.bfloat16)))
    r = R.f32_to_bf16(ties)
    assert np.array_equal(r & 1, np.zeros_like(r)) and (r[1::2] == r[0::2] + 2).all()  # down, then up, to even
    assert R.f32_to_bf16(np.array([BF16_MAX + 2.0 ** 119], dtype=F32))[0] == 0x7f80  # the tie to infinity
    q = R.f32_to_bf16(np.array([np.nan, -np.nan], dtype=F32))
    assert np.isnan(R.bf16_to_f32(q)).all()


# ------------------------------------------------------------------------------ elementwise
def _ew_inputs(bf16, seed):
    """n = 3 * 5 * 14 elements with every ordered pair of SPECIALS at the front of (a, s)"""
    rng = np.random.RandomState(seed)
    n, C, inner = 3 * 5 * 14 * 4, 5, 14
    mk = (lambda m: bf16_values(rng, m)) if bf16 else (lambda m: rng.standard_normal(m).astype(F32))
    a, s, g2, y = mk(n), mk(n), mk(n), mk(n)
    k = len(SPECIALS)
    a[:k * k] = np.repeat(SPECIALS, k)
    s[:k * k] = np.tile(SPECIALS, k)
    y[:k * k] = np.tile(SPECIALS, k)
    ba, bs = mk(C), mk(C)
    return n, C, inner, a, s, g2, y, ba, bs


def _eq(ref, tt, bf16, what):
    """reference (float32 values) vs a torch result: NaN as NaN, zeros by value, else bit-equal"""
    if bf16:
        assert tt.dtype == torch.bfloat16
        got, want = R.f32_to_bf16(ref), bits_of(tt)
        nan = np.isnan(R.bf16_to_f32(want))
        assert np.array_equal(np.isnan(R.bf16_to_f32(got)), nan), what
        zero = R.bf16_to_f32(want) == 0
        assert np.array_equal(R.bf16_to_f32(got) == 0, zero), what
        keep = ~nan & ~zero
        assert np.array_equal(got[keep], want[keep]), what
    else:
        assert tt.dtype == torch.float32
        R.assert_same(np.asarray(ref, dtype=F32), tt.numpy(), what)


@pytest.mark.parametrize("bf16", [False, True])
def test_elementwise_refs_match_torch(bf16):
    n, C, inner, a, s, g2, y, ba, bs = _ew_inputs(bf16, 5)
    dt = torch.bfloat16 if bf16 else torch.float32
    shape = (n // (C * inner), C, inner)
    T = lambda v: t32(v).view(shape)  # noqa: E731
    B = lambda v: t32(v).view(1, C, 1)  # noqa: E731
    flat = lambda t: t.reshape(-1)  # noqa: E731
    for use_a, use_s in [(True, True), (True, False), (False, True), (False, False)]:
        pa = T(a) + B(ba) if use_a else T(a) + 0.0
        ps = T(s) + B(bs) if use_s else T(s) + 0.0
        _eq(R.add_bias_relu_ref(a, ba if use_a else None, s, bs if use_s else None, C, inner),
            flat(torch.relu(pa + ps).to(dt)), bf16, "add_bias_relu %s %s" % (use_a, use_s))
        for relu in (0, 1):
            _eq(R.bias_act_ref(a, ba if use_a else None, C, inner, relu),
                flat((torch.relu(pa) if relu else pa).to(dt)), bf16, "bias_act relu=%d %s" % (relu, use_a))
    zero = torch.zeros(n)
    _eq(R.relu_mask_ref(a, None, y), torch.where(t32(y) > 0, t32(a), zero).to(dt), bf16, "relu_mask")
    _eq(R.relu_mask_ref(a, g2, y), torch.where(t32(y) > 0, t32(a) + t32(g2), zero).to(dt), bf16, "relu_mask g2")
    # the reference lets NaN through the forward and cuts the gradient at a NaN or -0.0 activation
    r = R.add_bias_relu_ref(a, None, s, None, C, inner)
    assert np.isnan(r[:len(SPECIALS)]).all()
    k = len(SPECIALS)
    m = R.relu_mask_ref(np.ones(k * k, dtype=F32), None, y[:k * k])
    assert np.array_equal(m != 0, np.tile(SPECIALS, k) > 0) and (m[np.isnan(y[:k * k])] == 0).all()
    # torch's own backward passes the gradient at a NaN activation: the documented difference
    tb = torch.ops.aten.threshold_backward(torch.ones(k * k), t32(y[:k * k]), 0.0).numpy()
    assert (tb[np.isnan(y[:k * k])] == 1).all()


def test_channel_of_element():
    """the channel of element i is (i // inner) % C: NCHW (inner = H*W) and NHWC (inner = 1) views
    of one tensor give the same sums as torch's broadcast"""
    rng = np.random.RandomState(1)
    N, C, H, W = 2, 6, 3, 5
    x, b = rng.standard_normal((N, C, H, W)).astype(F32), rng.standard_normal(C).astype(F32)
    want = (t32(x) + t32(b).view(1, C, 1, 1)).numpy()
    got = R.bias_act_ref(x.reshape(-1), b, C, H * W, 0).reshape(N, C, H, W)
    assert np.array_equal(got, want)
    got = R.bias_act_ref(x.transpose(0, 2, 3, 1).reshape(-1), b, C, 1, 0).reshape(N, H, W, C)
    assert np.array_equal(got.transpose(0, 3, 1, 2), want)


# ------------------------------------------------------------------------------ max pool
def _torch_pool(x, k, s, p):
    """F.max_pool2d on the NHWC array -> (y [n, ho, wo, c], window position [n, ho, wo, c])"""
    n, h, w, c = x.shape
    y, flat = Fn.max_pool2d(t32(x).permute(0, 3, 1, 2), k, s, p, return_indices=True)
    ho, wo = y.shape[2:]
    iy, ix = flat // w, flat % w
    oy = torch.arange(ho).view(1, 1, ho, 1)
    ox = torch.arange(wo).view(1, 1, 1, wo)
    pos = (iy - (oy * s - p)) * k + (ix - (ox * s - p))
    return y.permute(0, 2, 3, 1).numpy(), pos.permute(0, 2, 3, 1).numpy(), flat


@pytest.mark.parametrize("family", ["ties", "negative", "special"])
@pytest.mark.parametrize("k,s,p,h,w", R.GEOMS)
def test_maxpool_refs_match_torch(k, s, p, h, w, family):
    rng = np.random.RandomState(k * 100 + s * 10 + h)
    n, c = 2, 5
    x = R.pool_input(family, rng, n, h, w, c, k)
    y, idx = R.maxpool_ref(x, k, s, p)
    ty, tpos, tflat = _torch_pool(x, k, s, p)
    assert R.pool_out(h, w, k, s, p) == ty.shape[1:3]
    R.assert_same(y, ty, "maxpool_ref values")
    assert np.array_equal(idx & 0x7f, tpos), "maxpool_ref index"
    assert np.array_equal((idx & 0x80) != 0, ty > 0)
    if family == "special":
        assert np.isneginf(y).any() and (h * w < 9 or np.isnan(y).any())
    # backward, relu = 0: integer gradients, every float32 sum exact -> torch's float64 result casts
    # to the same bits
    gy = rng.randint(-8, 9, y.shape).astype(F32)
    tg = torch.ops.aten.max_pool2d_with_indices_backward(
        t32(gy).permute(0, 3, 1, 2).double(), t32(x).permute(0, 3, 1, 2).double(), [k, k], [s, s], [p, p], [1, 1],
        False, tflat).permute(0, 2, 3, 1)
    gx = R.maxpool_bwd_ref(gy, idx, x.shape, k, s, p, relu=0)
    assert np.array_equal(gx, tg.float().numpy())
    # relu = 1 == torch's backward, then the mask of the ReLU that fed the pool
    gx1 = R.maxpool_bwd_ref(gy, idx, x.shape, k, s, p, relu=1)
    want = torch.where(t32(x) > 0, tg, torch.zeros_like(tg)).float().numpy()
    assert np.array_equal(gx1, want)


def test_maxpool_bwd_ref_order_is_oy_ox():
    """Wide exponent spread, 3x3 stride 1 with the maxima on a stride-2 lattice (a lattice pixel collects
    up to 9 windows): the reference equals a per-pixel sum of its windows in (oy, ox) order added one
    float32 at a time, and the reverse order gives other bits."""
    k, s, p, n, h, w, c = 3, 1, 1, 1, 6, 7, 3
    x = np.zeros((n, h, w, c), dtype=F32)
    x[:, ::2, ::2, :] = 1.0   # maxima on a stride-2 lattice: each collects up to 9 windows
    y, idx = R.maxpool_ref(x, k, s, p)
    gy = R.spread_grad(np.random.RandomState(4), y.shape)
    gx = R.maxpool_bwd_ref(gy, idx, x.shape, k, s, p, relu=0)
    want = np.zeros_like(gx)
    ho, wo = y.shape[1:3]
    for iy in range(h):
        for ix in range(w):
            for ch in range(c):
                acc = F32(0)
                for oy in range(ho):
                    for ox in range(wo):
                        pos = int(idx[0, oy, ox, ch] & 0x7f)
                        if (oy * s - p + pos // k, ox * s - p + pos % k) == (iy, ix):
                            acc = F32(acc + gy[0, oy, ox, ch])
                want[0, iy, ix, ch] = acc
    assert np.array_equal(gx, want)
    # pixel (2, 2) collects windows (2, 2), (2, 3), (3, 2), (3, 3) in that order: 2^24 + 1 + 1 + 1 stays
    # 2^24 in float32 (each add is a tie to even), while 1 + 1 + 1 + 2^24 rounds to 2^24 + 4
    gy = np.ones(y.shape, dtype=F32)
    gy[0, 2, 2, :] = 2.0 ** 24
    assert (R.maxpool_bwd_ref(gy, idx, x.shape, k, s, p, relu=0)[0, 2, 2] == 2.0 ** 24).all()
    assert (R.maxpool_bwd_ref(gy, idx, x.shape, k, s, p, relu=0, reverse=True)[0, 2, 2] == 2.0 ** 24 + 4).all()


def test_maxpool_rules_on_hand_built_planes():
    """One 4 x 4 plane per rule, 2 x 2 windows of stride 2 and a 3 x 3 padded window; torch agrees
    with each expectation."""
    inf, nan = np.inf, np.nan
    plane = np.array([[1, 1, -inf, -inf],
                      [1, 1, -inf, -inf],
                      [nan, 5, 0, -2],
                      [7, nan, -2, 0]], dtype=F32).reshape(1, 4, 4, 1)
    y, idx = R.maxpool_ref(plane, 2, 2, 0)
    # tie: first wins (0, bit 7); all -inf: first valid position 0, no bit 7; NaN: the last one (3);
    # maximum 0: first zero, bit 7 clear
    assert np.array_equal(idx.reshape(2, 2), np.array([[0x80, 0], [3, 0]], dtype=np.uint8))
    assert y[0, 0, 0, 0] == 1 and np.isneginf(y[0, 0, 1, 0]) and np.isnan(y[0, 1, 0, 0]) and y[0, 1, 1, 0] == 0
    ty, tpos, _ = _torch_pool(plane, 2, 2, 0)
    R.assert_same(y, ty, "hand-built 2x2")
    assert np.array_equal(idx & 0x7f, tpos)
    # padded: an all -inf plane starts at the first position INSIDE the image (kh = kw = 1 -> 4)
    neg = np.full((1, 3, 3, 1), -inf, dtype=F32)
    y, idx = R.maxpool_ref(neg, 3, 2, 1)
    assert np.array_equal(idx.reshape(2, 2), np.array([[4, 3], [1, 0]], dtype=np.uint8))
    ty, tpos, _ = _torch_pool(neg, 3, 2, 1)
    assert np.array_equal(idx & 0x7f, tpos) and np.isneginf(ty).all()
    # backward with relu: the zero-maximum and NaN windows are dropped, the -inf one too
    gy = np.arange(1, 5, dtype=F32).reshape(1, 2, 2, 1)
    y, idx = R.maxpool_ref(plane, 2, 2, 0)
    g0 = R.maxpool_bwd_ref(gy, idx, plane.shape, 2, 2, 0, relu=0).reshape(4, 4)
    g1 = R.maxpool_bwd_ref(gy, idx, plane.shape, 2, 2, 0, relu=1).reshape(4, 4)
    assert g0[0, 0] == 1 and g0[0, 2] == 2 and g0[3, 1] == 3 and g0[2, 2] == 4 and np.count_nonzero(g0) == 4
    assert g1[0, 0] == 1 and np.count_nonzero(g1) == 1
