"""Plain-numpy references of the epilogue entries of include/wam_hip.h (the kernels of
wam_amd/csrc/epilogue.hip), written from the header's contract sentences, and the two comparators
the GPU tests hold the kernels to.

Every reference takes `dt`: np.float64 is the high-precision form, np.float32 the emulated form --
the documented sequence of fp32 adds and divisions on numpy float32 arrays (numpy rounds each
operation to nearest even, as the GPU does without fast-math; no multiply-add appears in those
sequences). tests/test_epilogue_ref.py pins each reference to numpy / the float64 oracle.

Layouts (as the header): coefficient gradients band-major (band b: [items * C, n_b] at
items * C * off[b]); maps item-major [items, K] with band b at off[b]; band_max [groups, bands];
frames [group_items, frame_len]; src / band per frame pixel, dst / cband per packed coefficient.
"""
import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff
FLT_MAX = float(np.finfo(np.float32).max)
WORST = {}              # largest error / bound ratio seen by assert_within, per first word of `what`


# ------------------------------------------------------------------------------ comparators
def assert_within(got, ref, bound, what, exclude=None, max_excluded=0.01):
    """(a): |got - ref| <= bound per element (bound broadcastable; NaN exactly where ref has NaN).
    exclude: boolean mask of elements left to assert_bits (at most max_excluded of them).
    Prints and returns the largest error / bound ratio."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    keep = np.ones(ref.shape, dtype=bool)
    if exclude is not None:
        assert exclude.mean() <= max_excluded, "%s: %.3f of the elements excluded" % (what, exclude.mean())
        keep &= ~exclude
    g, r, b = got[keep], ref[keep], bound[keep]
    nan = np.isnan(r)
    assert np.array_equal(np.isnan(g), nan), "%s: NaN at other elements than the reference" % what
    assert not np.isnan(b[~nan]).any() and (b[~nan] >= 0).all(), "%s: bad bound" % what
    err = np.abs(g[~nan] - r[~nan])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / b[~nan])
    worst = float(ratio.max()) if ratio.size else 0.0
    key = what.split()[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("[epilogue] %s: max error / bound = %.3g over %d elements" % (what, worst, ratio.size))
    assert worst <= 1.0, "%s: error / bound = %.3g" % (what, worst)
    return worst


def assert_bits(got, ref, what, only=None):
    """(b): got equals the fp32-emulated reference bit for bit as values (NaN == NaN)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if only is not None:
        got, ref = got[only], ref[only]
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), "%s: %d of %d elements differ from the emulated reference, first at %s" % (
        what, (~same).sum(), same.size, np.argwhere(~same)[0])


def rel_bound(ref, rel=1e-12):
    """the bar of the float64 kernels: rel * max(1, |ref|.max()) (NaN ignored)."""
    r = np.abs(np.asarray(ref, dtype=np.float64))
    r = r[np.isfinite(r)]
    return rel * max(1.0, float(r.max()) if r.size else 0.0)


# ------------------------------------------------------------------------------ tables
def make_tables(rng, frame_len, maps_item_len, n_bands, mapped):
    """A synthetic injective mosaic: `mapped` random frame pixels <- distinct random coefficients;
    the other pixels are holes (src -1) and the other coefficients go nowhere (dst -1). Bands are
    contiguous coefficient ranges, as in a packed item. -> src, band, dst, cband (int32)."""
    assert mapped <= min(frame_len, maps_item_len)
    pix = rng.permutation(frame_len)[:mapped]
    coef = rng.permutation(maps_item_len)[:mapped]
    cuts = np.sort(rng.choice(np.arange(1, maps_item_len), n_bands - 1, replace=False)) if n_bands > 1 else []
    cband = np.searchsorted(np.asarray(cuts), np.arange(maps_item_len), side="right").astype(np.int32)
    src = np.full(frame_len, -1, dtype=np.int32)
    src[pix] = coef
    band = np.zeros(frame_len, dtype=np.int32)
    band[pix] = cband[coef]
    dst = np.full(maps_item_len, -1, dtype=np.int32)
    dst[coef] = pix
    return src, band, dst, cband


# ------------------------------------------------------------------------------ maps
def maps_ref(g, groups, group_items, C, band_offsets, dt=np.float64):
    """wam_subband_maps: maps[item, band-packed] = |((g0 + g1) + g2 ...) / C| and
    band_max[group, band] = max over the group's items (numpy's max: NaN propagates)."""
    items = groups * group_items
    nb = len(band_offsets) - 1
    K = band_offsets[-1]
    g = np.asarray(g)
    maps = np.empty((items, K), dtype=dt)
    bmax = np.empty((groups, nb), dtype=dt)
    for b in range(nb):
        n = band_offsets[b + 1] - band_offsets[b]
        gb = g[items * C * band_offsets[b]:items * C * band_offsets[b + 1]].reshape(items, C, n).astype(dt)
        acc = gb[:, 0]
        for c in range(1, C):
            acc = acc + gb[:, c]
        m = np.abs(acc / dt(C))
        maps[:, band_offsets[b]:band_offsets[b + 1]] = m
        bmax[:, b] = m.reshape(groups, group_items * n).max(axis=1)
    return maps, bmax


def maps_abs_sum(g, items, C, band_offsets):
    """sum_c |g_c| per map element (the scale of the maps bound), item-major."""
    nb = len(band_offsets) - 1
    out = np.empty((items, band_offsets[-1]))
    for b in range(nb):
        n = band_offsets[b + 1] - band_offsets[b]
        gb = np.asarray(g, dtype=np.float64)[items * C * band_offsets[b]:items * C * band_offsets[b + 1]]
        out[:, band_offsets[b]:band_offsets[b + 1]] = np.abs(gb.reshape(items, C, n)).sum(axis=1)
    return out


# ------------------------------------------------------------------------------ mosaic
def _mosaic_values(maps, band_max, src, band, s, group_items, normalize, dt):
    """value of every mosaic pixel for group s in dt: maps[(s, n), src[p]] (/ band_max[s, band[p]]);
    -> (valid pixel mask, values [group_items, valid pixels])."""
    valid = src >= 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = maps[s * group_items:(s + 1) * group_items][:, src[valid]].astype(dt)
        if normalize:
            v = v / band_max[s, band[valid]].astype(dt)[None, :]
    return valid, v


def _nan_to_num(v):
    """numpy's nan_to_num of float32 data (NaN -> 0, +-inf -> +-FLT_MAX) in the dtype of v"""
    return np.nan_to_num(v, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)


def frame_accumulate_ref(frame, maps, band_max, src, band, groups, group_items, normalize, emulate=False):
    """wam_frame_accumulate(_coef): for s in order frame[n, p] += fp64(term), term = the map value
    (/ band maximum). emulate: the term is the fp32 quotient widened (the contract); otherwise the
    float64 quotient. src[p] == -1 pixels are untouched. Returns a new float64 frame."""
    out = np.array(frame, dtype=np.float64).reshape(group_items, -1).copy()
    for s in range(groups):
        valid, v = _mosaic_values(maps, band_max, src, band, s, group_items, normalize,
                                  np.float32 if emulate else np.float64)
        with np.errstate(invalid="ignore"):
            out[:, valid] += v.astype(np.float64)
    return out


def frame_trapz_ref(prev, acc, maps, band_max, src, band, groups, k0, group_items, normalize, weights=None,
                    dt=np.float64):
    """wam_frame_trapz(_coef): for step k = k0 + s, G = nan_to_num(mosaic value (normalised)), 0 at
    src == -1; sequential: if k > 0: acc += (prev + G) / 2, prev = G; weighted: acc += w[s] * G.
    nan_to_num comes AFTER the normalising division. Returns new (prev, acc) in dt."""
    prev = np.array(prev, dtype=dt).reshape(group_items, -1).copy()
    acc = np.array(acc, dtype=dt).reshape(group_items, -1).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(groups):
            valid, v = _mosaic_values(maps, band_max, src, band, s, group_items, normalize, dt)
            G = np.zeros(prev.shape, dtype=dt)
            G[:, valid] = _nan_to_num(v)
            if weights is not None:
                acc = acc + dt(weights[s]) * G
            else:
                if k0 + s > 0:
                    acc = acc + (prev + G) / dt(2)
                prev = G
    return prev, acc


def cube_ref(prev, acc, maps, src, groups, k0, group_items, mode, n_total=1.0, weights=None, dt=np.float64):
    """wam_cube_accumulate: value = maps[(s, n), src[p]] (0 at src == -1), for s in order
    mode 0: acc = (acc + value) / n_total; mode 1: acc += w[s] * value; mode 2: the sequential
    trapezoid of frame_trapz_ref. prev may be None in modes 0 and 1. Returns new (prev, acc)."""
    acc = np.array(acc, dtype=dt).reshape(group_items, -1).copy()
    prev = None if prev is None else np.array(prev, dtype=dt).reshape(group_items, -1).copy()
    valid = src >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(groups):
            v = np.zeros(acc.shape, dtype=dt)
            v[:, valid] = maps[s * group_items:(s + 1) * group_items][:, src[valid]].astype(dt)
            if mode == 0:
                acc = (acc + v) / dt(n_total)
            elif mode == 1:
                acc = acc + dt(weights[s]) * v
            else:
                v = _nan_to_num(v)
                if k0 + s > 0:
                    acc = acc + (prev + v) / dt(2)
                prev = v
    return prev, acc  # modes 0 and 1 leave the trapezoid state as it came


# ------------------------------------------------------------------------------ streams
def accumulate_ref(acc, src, groups, scale=0.0, dt=np.float64):
    """wam_accumulate_f32: acc += src[s] for s in order, then (scale != 0) acc = acc / scale --
    the division takes the whole accumulator, the incoming acc included."""
    a = np.array(acc, dtype=dt).copy()
    src = np.asarray(src).reshape(groups, -1)
    for s in range(groups):
        a = a + src[s].astype(dt)
    if scale != 0:
        a = a / dt(scale)
    return a


def trapz_stream_ref(prev, acc, src, groups, k0, weights=None, dt=np.float64):
    """wam_trapz_f32: G_s = src[s] (no nan_to_num); sequential or weighted as frame_trapz_ref;
    dt float64 is also the kernel's own fp64-accumulator form. prev may be None with weights."""
    a = np.array(acc, dtype=dt).copy()
    p = None if prev is None else np.array(prev, dtype=dt).copy()
    src = np.asarray(src).reshape(groups, -1)
    for s in range(groups):
        G = src[s].astype(dt)
        if weights is not None:
            a = a + dt(weights[s]) * G
        else:
            if k0 + s > 0:
                a = a + (p + G) / dt(2)
            p = G
    return p, a


def sigma_ref(x, items, item_stride, length, spread):
    """wam_item_sigma: fp32(spread) * (max - min) of x_i[0:length] in fp32, NaN propagating."""
    xv = np.asarray(x, dtype=np.float32)[:items * item_stride].reshape(items, item_stride)[:, :length]
    with np.errstate(invalid="ignore"):
        return np.float32(spread) * (xv.max(axis=1) - xv.min(axis=1))


# ------------------------------------------------------------------------------ .scales
def _lin_axis(n_out, n_in):
    """taps and weight of a half-pixel-centre linear upsampling axis, clamped to the edge"""
    sv = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
    sv = np.maximum(sv, 0.0)
    i0 = np.minimum(np.floor(sv).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, sv - i0


def bilinear_up(a, size):
    """cv2 INTER_LINEAR upsampling of [items, h, w] float64 blocks to size x size"""
    if a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError("bilinear_up of an empty block %s" % (a.shape,))
    y0, y1, fy = _lin_axis(size, a.shape[1])
    x0, x1, fx = _lin_axis(size, a.shape[2])
    top = a[:, y0][:, :, x0] * (1 - fx) + a[:, y0][:, :, x1] * fx
    bot = a[:, y1][:, :, x0] * (1 - fx) + a[:, y1][:, :, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def reproject_ref(avg, levels, approx):
    """wam_reproject_scales: out[item, j] = up(H) + up(V) + up(D) of level j's quadrants, split at
    s = int(size / 2**(j+1)), e = int(size / 2**j); with approx out[item, levels] = up(avg[:e, :e]),
    e = int(size / 2**levels). An empty quadrant raises, as the reference does."""
    avg = np.asarray(avg, dtype=np.float64)
    n, size = avg.shape[0], avg.shape[1]
    out = np.zeros((n, levels + (1 if approx else 0), size, size))
    for j in range(levels):
        e, s = int(size / 2 ** j), int(size / 2 ** (j + 1))
        out[:, j] = (bilinear_up(avg[:, :s, s:e], size) + bilinear_up(avg[:, s:e, :s], size)
                     + bilinear_up(avg[:, s:e, s:e], size))
    if approx:
        e = int(size / 2 ** levels)
        out[:, levels] = bilinear_up(avg[:, :e, :e], size)
    return out
