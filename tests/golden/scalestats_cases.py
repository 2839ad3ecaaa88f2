"""Cases shared by make_scalestats_goldens.py and the scale-statistics tests: inputs regenerated from
RandomState seeds (identical under numpy 1.26 and 2.x), never stored."""
import numpy as np

GOLDENS = "scalestats_goldens.npz"
SIZES = ("maximal", "minimal")

# name: (H, J, N, seed, the `size` values whose variance MAP is stored; the mean is stored for both).
# Detail block sides: s30 15 / 8 / 4 (approximation 3); s8 4 / 2 / 1 (under "minimal" T = 1, the zoom's
# m = 1 case); s7 4 / 2; s100 50 / 25 / 13 and s225 113 / 56 / 28 / 14 (non-dyadic zoom factors: a coordinate
# formula other than scipy's breaks the bar there); s64j1 a single level (the variance is exactly 0.0);
# s224n3 the flagship size, results only: its 112^2 "maximal" maps are not stored, its 28^2 "minimal" ones are
# -- there (and at s225 "minimal") scipy's coordinate of the last output index rounds above n - 1 and the
# last row and column of the resized 56^2 (28^2) level are 0.
LEVEL_CASES = {
    "s32": (32, 3, 1, 3201, SIZES),
    "s30": (30, 3, 1, 3001, SIZES),
    "s8": (8, 3, 1, 801, SIZES),
    "s7": (7, 2, 1, 701, SIZES),
    "s100": (100, 3, 1, 10001, SIZES),
    "s225": (225, 4, 1, 22501, SIZES),
    "s64j1": (64, 1, 1, 6401, SIZES),
    "s224n3": (224, 3, 3, 22401, ("minimal",)),
    "s32n5": (32, 3, 5, 3205, SIZES),
}
RANK_CASES = ("s224n3", "s32n5")       # rank_images over the case's N maps, both sizes
RANK_MIN_GAP = 1e-9                    # neighbouring mean variances differ by more than this, relative


def make_maps(H, N, seed):
    """N WAM-like maps [N, H, H] float64: signed (the sums take |v|), energy growing towards the
    coarse corner and differing between images, so that levels and images disagree."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:H] / float(H)
    out = []
    for i in range(N):
        envelope = 0.2 + np.exp(-(2.0 + i) * (xx + yy))
        out.append(rs.standard_normal((H, H)) * envelope * rs.uniform(0.5, 2.0))
    return np.stack(out)


def level_key(kind, name, size=None):
    return "%s_%s" % (kind, name) if size is None else "%s_%s_%s" % (kind, name, size)


# ---- mask agreement: M maps of `len` pixels quantised to the integers 0 .. 9, so every threshold is tied
PERCENTAGES = (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.0, 1.0)
IOU_M = (2, 3, 5)
IOU_LEN = (20, 63, 64, 65, 1000)
IOU_CHUNKED = ("m17_l65", 17, 65)      # one M above the kernel's bound of 16: the chunked path
IOU_TWINS = ("twins_l65", 65)          # two identical maps: IoU 1.0 at every percentage


def iou_cases():
    """name -> (M, len, seed)"""
    out = {}
    for M in IOU_M:
        for n in IOU_LEN:
            out["m%d_l%d" % (M, n)] = (M, n, 1000 * M + n)
    out[IOU_CHUNKED[0]] = (IOU_CHUNKED[1], IOU_CHUNKED[2], 1765)
    return out


def make_iou_maps(M, n, seed):
    return np.random.RandomState(seed).randint(0, 10, size=(M, n)).astype(np.float64)


def make_twins(n):
    m = make_iou_maps(1, n, 4242)
    return np.concatenate([m, m])
