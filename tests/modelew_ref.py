"""Plain-numpy references of the wam_ew_* entries of include/wam_hip.h (the kernels of
wam_amd/csrc/model_ew.hip), written from the header's contract sentences, the bf16 storage
helpers, and the shared case data of tests/test_modelew_ref.py (CPU, against torch) and
tests/test_gpu_modelew.py (the kernels at the C ABI).

No torch in the arithmetic: every sum is a numpy float32 add (rounded to nearest even, as the GPU
adds without fast-math). The contract has no multiply, so nothing can contract into a
multiply-add and the results are reproducible bit for bit. All references take and return
float32 arrays -- the value a kernel holds after unpacking its storage type; `store` rounds to
the storage type (bf16: round to nearest even, the kernels' single rounding on the store).

Special values (the contract):
  forward ReLU   v < 0 ? 0 : v -- NaN propagates, as torch.relu / clamp_min do; -0.0 may come out as
                 either zero (the tests compare zeros by value)
  ReLU mask      y > 0 ? g : 0 -- 0 where y is -0.0, negative or NaN. This is the header's
                 contract and differs from torch's threshold_backward (`y <= 0 ? 0 : g`), which
                 lets the gradient through where y is NaN.
  max pool       scan order kh * k + kw; a candidate replaces the running maximum when it is
                 greater or NaN, so the first of equal maxima wins, the last NaN in scan order
                 wins, and a window of -inf only keeps its start index, the first valid position.
                 Bit 7 of the index byte is set iff the maximum is > 0 (not for NaN).
"""
import numpy as np

F32 = np.float32

# (k, stride, pad, h, w) of the max-pool tests
GEOMS = [
    (3, 2, 1, 7, 6),      # the stem's geometry at a small odd size: KC = 3 forward, W2 backward
    (3, 1, 1, 5, 4),      # up to 9 windows per pixel: KC = 3 forward, looped backward
    (3, 1, 1, 3, 70),     # wo = 70: with 4 channel vectors per pixel 280 threads, a second workgroup in x
    (2, 2, 0, 5, 4),      # the last row lies in no window
    (2, 1, 0, 3, 3),
    (2, 3, 0, 8, 7),      # stride > k and not a power of two: uncovered pixels, the a / d division
    (5, 3, 2, 9, 11),     # stride 3 again, windows overlap (W2 backward with ceil(5 / 3) = 2)
    (5, 1, 2, 6, 6),      # up to 25 windows per pixel
    (7, 2, 3, 9, 8),
    (11, 4, 5, 12, 13),   # the largest window: positions up to 120, 120 | 0x80 = 248
    (1, 1, 0, 2, 2),      # the identity
    (1, 2, 0, 3, 3),      # subsampling: odd rows / columns in no window
    (4, 2, 2, 5, 5),      # 2 * pad == k: the first window has two padded rows
    (3, 2, 1, 1, 1),      # a single pixel
]


# ------------------------------------------------------------------------------ bf16 storage
def bf16_to_f32(bits):
    """uint16 bf16 patterns -> float32 (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def f32_to_bf16(v):
    """float32 -> uint16 bf16 patterns, round to nearest even; NaN stays NaN (quiet bit set)."""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def store(v, bf16):
    """What a kernel's store leaves in memory, as float32 values: v itself, or v rounded to bf16."""
    v = np.asarray(v, dtype=F32)
    return bf16_to_f32(f32_to_bf16(v)) if bf16 else v


def same(got, ref):
    """Elementwise: equal as values (so bit-equal unless both are zeros) or both NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    return (got == ref) | (np.isnan(got) & np.isnan(ref))


def assert_same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    ok = same(got, ref)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d elements differ from the reference, first at %s: got %r, reference %r" % (
            what, (~ok).sum(), ok.size, i, got[i], ref[i]))


# ------------------------------------------------------------------------------ elementwise
def _channel(n, C, inner):
    return (np.arange(n, dtype=np.int64) // inner) % C


def _biased(x, b, ch):
    x = np.asarray(x, dtype=F32)
    return x + (F32(0) if b is None else np.asarray(b, dtype=F32)[ch])


def _relu(v):
    return np.where(v < 0, F32(0), v).astype(F32)


def bias_act_ref(y, b, C, inner, relu):
    """relu ? relu(y + b[c]) : y + b[c] over a flat array, c = (i // inner) % C; b may be None (0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = _biased(y, b, _channel(len(y), C, inner))
        return _relu(v) if relu else v


def add_bias_relu_ref(a, ba, s, bs, C, inner):
    """relu((a + ba[c]) + (s + bs[c])) in the header's association."""
    ch = _channel(len(a), C, inner)
    with np.errstate(invalid="ignore", over="ignore"):
        return _relu(_biased(a, ba, ch) + _biased(s, bs, ch))


def relu_mask_ref(g1, g2, y):
    """y > 0 ? g1 (+ g2) : 0 -- 0 where y is -0.0, negative or NaN (torch's threshold_backward
    passes the gradient at a NaN y; the header does not)."""
    g1 = np.asarray(g1, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        g = g1 if g2 is None else g1 + np.asarray(g2, dtype=F32)
        return np.where(np.asarray(y, dtype=F32) > 0, g, F32(0)).astype(F32)


# ------------------------------------------------------------------------------ max pool
def pool_out(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _valid(o, s, p, k, size):
    """window o along one axis: its origin and the range of window positions inside the image"""
    x0 = o * s - p
    return x0, max(0, -x0), min(k, size - x0)


def maxpool_ref(x, k, s, p):
    """x [n, h, w, c] float32 -> (y [n, ho, wo, c] float32, idx uint8). idx = kh * k + kw of the
    maximum, bit 7 set iff the maximum is > 0; rules in the module docstring."""
    x = np.asarray(x, dtype=F32)
    n, h, w, c = x.shape
    ho, wo = pool_out(h, w, k, s, p)
    y = np.empty((n, ho, wo, c), dtype=F32)
    idx = np.empty((n, ho, wo, c), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for oy in range(ho):
            y0, ky0, ky1 = _valid(oy, s, p, k, h)
            for ox in range(wo):
                x0, kx0, kx1 = _valid(ox, s, p, k, w)
                m = np.full((n, c), -np.inf, dtype=F32)
                pos = np.full((n, c), ky0 * k + kx0, dtype=np.int64)
                for ky in range(ky0, ky1):
                    for kx in range(kx0, kx1):
                        v = x[:, y0 + ky, x0 + kx, :]
                        take = (v > m) | np.isnan(v)
                        m = np.where(take, v, m)
                        pos = np.where(take, ky * k + kx, pos)
                y[:, oy, ox, :] = m
                idx[:, oy, ox, :] = (pos | np.where(m > 0, 0x80, 0)).astype(np.uint8)
    return y, idx


def maxpool_bwd_ref(gy, idx, shape, k, s, p, relu, reverse=False):
    """gx [n, h, w, c] float32: every window adds its gy to the pixel its index points at, windows
    taken in (oy, ox) order, float32 adds from 0; with relu a window whose bit 7 is clear adds
    nothing. reverse: the opposite window order (for the test that shows the order matters)."""
    gy = np.asarray(gy, dtype=F32)
    n, h, w, c = shape
    ho, wo = pool_out(h, w, k, s, p)
    assert gy.shape == (n, ho, wo, c) and idx.shape == gy.shape and idx.dtype == np.uint8
    gx = np.zeros((n, h, w, c), dtype=F32)
    nn, cc = np.meshgrid(np.arange(n), np.arange(c), indexing="ij")
    order = [(oy, ox) for oy in range(ho) for ox in range(wo)]
    for oy, ox in (reversed(order) if reverse else order):
        b = idx[:, oy, ox, :].astype(np.int64)
        pos = b & 0x7f
        iy, ix = oy * s - p + pos // k, ox * s - p + pos % k
        live = (b & 0x80) != 0 if relu else np.ones_like(b, dtype=bool)
        # one term per (image, channel) lane and step: the targets of one step are distinct
        gx[nn[live], iy[live], ix[live], cc[live]] += gy[:, oy, ox, :][live]
    return gx


# ------------------------------------------------------------------------------ shared inputs
LEVELS = np.array([0.25, 0.5, 1.0, 1.0, 2.0, -0.5, -1.5], dtype=F32)   # exact in bf16


def pool_input(family, rng, n, h, w, c, k):
    """The three input families of the pool tests, [n, h, w, c] float32 with bf16-exact values:
    'ties'      a few levels with 30 % exact zeros: equal maxima and zero maxima are frequent
    'negative'  every value below zero: bit 7 is clear on every maximum
    'special'   'ties' plus planes of -inf (all of image 0 in every third channel, a corner block
                of image 1 wide enough to hold whole windows) and 6 % scattered NaN, some of them
                inside the -inf regions"""
    x = LEVELS[rng.randint(0, len(LEVELS), (n, h, w, c))]
    x = np.where(rng.uniform(size=x.shape) < 0.3, F32(0), x).astype(F32)
    if family == "negative":
        return (-np.abs(x) - F32(0.125)).astype(F32)
    if family == "special":
        x[0, :, :, ::3] = -np.inf
        x[n - 1, :k + 2, :k + 2, :] = -np.inf
        x[rng.uniform(size=x.shape) < 0.06] = np.nan
    else:
        assert family == "ties"
    return x


def spread_grad(rng, shape):
    """Gradients +-(1 + r / 128) 2^e, e in [-20, 20] (bf16-exact, 8 significant bits): two terms more
    than 17 binades apart no longer add exactly in float32, so a sum of a few of them depends on
    the order of the adds."""
    m = 1.0 + rng.randint(0, 128, shape) / 128.0
    sign = np.where(rng.uniform(size=shape) < 0.5, -1.0, 1.0)
    return (sign * m * 2.0 ** rng.randint(-20, 21, shape)).astype(F32)
