"""numpy restatement of the reference's scale statistics (top-level utils.py) and mask agreement
(compare_iou_models.ipynb), operation by operation in float64, and the error bars of the device tests.

The resize is scipy.ndimage.zoom(block, T / n, order=1)[:T, :T] restated (scipy is not needed to run
this): output length m = int(round(n * (T / n))), zoom = (n - 1) / (m - 1) (1 when m == 1), output
index o reads cc = zoom * o; i0 = floor(cc); weights w0 = 1 - (cc - i0) and w1 = 1 - w0 (scipy derives
the last weight from the others); value = ((v00 * w0r) * w0c + (v01 * w0r) * w1c) + ... in tap order,
rows outer. A tap at n has weight 0 (scipy reads its mirror image n - 2). A coordinate that rounds
above n - 1 -- the last index of some non-dyadic factors -- is out of bounds: that row / column of
the output is cval = 0 (mode 'constant'). tests/test_scalestats_ref.py checks all of it against what
scipy itself produced, bit for bit.
"""
import numpy as np

U = 2.0 ** -53


def detail_sides(H, J):
    return [H // 2 ** j - H // 2 ** (j + 1) for j in range(J)]


def diagonal(wam, J):
    """[level_0, ..., level_{J-1}, approx] blocks of a square map."""
    H = wam.shape[0]
    out = [wam[H // 2 ** (j + 1):H // 2 ** j, H // 2 ** (j + 1):H // 2 ** j] for j in range(J)]
    out.append(wam[:H // 2 ** J, :H // 2 ** J])
    return out


def abs_sums(wam, J):
    return np.array([np.sum(np.abs(b)) for b in diagonal(wam, J)])


def shares(wam, J):
    s = abs_sums(wam, J)
    s /= np.sum(s)
    return s


def target_side(H, J, size):
    sizes = detail_sides(H, J)
    if size == "maximal":
        return max(sizes)
    if size == "minimal":
        return min(sizes)
    raise ValueError("size must be 'maximal' or 'minimal'")


def zoom_length(n, T):
    return int(round(n * (T / n)))


def _axis(n, m, T, coord=None):
    o = np.arange(T, dtype=np.float64)
    if coord is None:
        zoom = (n - 1) / (m - 1) if m > 1 else 1.0
        cc = zoom * o
    else:
        cc = coord(o, n, m)
    inside = ~(cc > n - 1)
    fl = np.floor(cc)
    i0 = np.where(inside, fl, 0).astype(np.int64)
    i1 = np.where(i0 + 1 < n, i0 + 1, n - 2 if n > 1 else 0)
    w0 = 1.0 - (cc - fl)
    w1 = 1.0 - w0
    return i0, i1, w0, w1, inside


def zoom_block(block, T, coord=None):
    """scipy.ndimage.zoom(block, T / n, order=1)[:T, :T] of a square block. coord replaces the
    coordinate formula (the mutants of the tests)."""
    n = block.shape[0]
    m = zoom_length(n, T)
    if m < T:
        raise ValueError("all input arrays must have the same shape")
    i0, i1, w0, w1, inside = _axis(n, m, T, coord)
    t = np.zeros((T, T))
    for ia, wa in ((i0, w0), (i1, w1)):
        for ib, wb in ((i0, w0), (i1, w1)):
            t = t + (block[np.ix_(ia, ib)] * wa[:, None]) * wb[None, :]
    t[~inside, :] = 0.0
    t[:, ~inside] = 0.0
    return t


def variance_map(wam, J, size="maximal", coord=None):
    T = target_side(wam.shape[0], J, size)
    stack = np.stack([zoom_block(b, T, coord) for b in diagonal(wam, J)[:J]], axis=0)
    return np.var(stack, axis=0)


def mean_variance(wam, J, size="maximal"):
    return float(np.mean(variance_map(wam, J, size)))


def rank(maps, J, size="maximal"):
    r = [{"image_index": i, "mean_pixelwise_variance": mean_variance(m, J, size)} for i, m in enumerate(maps)]
    r.sort(key=lambda x: x["mean_pixelwise_variance"], reverse=True)
    return r


# ---- mask agreement

def highest_percentage(gray, p):
    flat = gray.flatten()
    t = flat[np.argsort(flat)[::-1][int(len(flat) * p) - 1]]
    return gray >= t


def pair_counts(maps, percentages):
    """(inter, uni) int64 [Q, M (M - 1) / 2], pairs (i < j) in lexicographic order."""
    M = len(maps)
    inter, uni = [], []
    for p in percentages:
        masks = [highest_percentage(m, p) for m in maps]
        inter.append([np.logical_and(masks[i], masks[j]).sum() for i in range(M) for j in range(i + 1, M)])
        uni.append([np.logical_or(masks[i], masks[j]).sum() for i in range(M) for j in range(i + 1, M)])
    return np.array(inter, dtype=np.int64), np.array(uni, dtype=np.int64)


def mean_iou(inter, uni):
    return np.array([np.mean([i / u if u != 0 else 0 for i, u in zip(iq, uq)]) for iq, uq in zip(inter, uni)])


# ---- error bars of the device tests (u = 2^-53), derived, not tuned

def abs_sum_rtol(n_elements):
    """Any two summation orders of n non-negative doubles differ by at most 2 (n - 1) u relative;
    (2 n + 8) u leaves room for the roundings of |v| (none) and of the final adds."""
    return (2 * n_elements + 8) * U


def var_atol(J, wam):
    """With scipy's coordinates followed bit for bit, each side makes at most about 60 + 8 J
    roundings per pixel, each of size u * max(map^2)."""
    return (128 + 16 * J) * U * float(np.max(np.asarray(wam) ** 2))


def mean_var_atol(J, wam, T, mean_var):
    """The variance bar plus the reordering of the T^2-term mean: 2 T^2 u relative."""
    return var_atol(J, wam) + 2 * T * T * U * abs(mean_var)
