"""Cases shared by make_analyzer_goldens.py and the analyzer tests: inputs regenerated from
RandomState seeds (identical under numpy 1.26 and 2.x), never stored."""
import numpy as np

GOLDENS = "analyzer_goldens.npz"
QS = (0.0, 0.3, 0.7, 0.95, 1.0)
EPS = 0.1
# name: (size, J, seed, the channels whose pixels are stored (all three are computed), the stored quantiles)
PARTIAL = {
    "s32": (32, 2, 3201, (0, 1, 2), QS),
    "s64": (64, 3, 6401, (0, 1, 2), QS),
}
# the quirk-quantised uint8 image at the flagship size: one channel stored (the size limit), mn / mx span all three
QUIRK = {"s224": (224, 3, 22401, (2,), (0.3, 0.9)), "s64u": (64, 3, 6403, (0, 1, 2), (0.3, 0.95))}
LEVELS = {"s32": (32, 2, 3202, (0, 1, 2)), "s64": (64, 3, 6402, (0, 1, 2))}


def make_image(size, seed):
    """show()'s output: HWC float32 in [0, 1] -- smooth structure plus noise, so every scale carries energy."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size] / float(size)
    base = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + c) * np.cos(4.0 * yy - c) for c in range(3)], axis=2)
    img = base + 0.1 * rs.standard_normal((size, size, 3))
    return np.clip(img, 0.0, 1.0).astype(np.float32)


def make_map(size, seed):
    """A WAM-like map: float64, strictly positive, all values distinct (asserted), not symmetric."""
    rs = np.random.RandomState(seed + 7)
    m = rs.uniform(0.05, 1.0, (size, size)) * (1.0 + np.arange(size)[None, :] / size)
    assert np.unique(m).size == m.size and not np.array_equal(m, m.T)
    return m


def key(kind, name, q=None):
    return "%s_%s" % (kind, name) if q is None else "%s_%s_q%03d" % (kind, name, int(round(100 * q)))


# End to end (tests/test_gpu_analyzer.py): 3 images of 64 x 64 (the default transform's resize path), haar J=3,
# testmodels.TinySmooth2D(seed=E2E_MODEL_SEED). Along E2E_QS the CPU restatement's arg-max classes are
# [0, 0, 0, 0, 3, 3, 0], [0, 0, 0, 3, 3, 0, 3] and [0, 0, 0, 3, 0, 4, 3] and the top two logits are at least
# 0.075 apart at every (image, quantile): 750 times the 1e-4 bar on the probabilities. Labels: 0 is image 0's
# own prediction at both ends, 3 is predicted for image 1 in the middle (first and last hit are not the ends),
# 7 is never predicted (the None tuple). With the reference's own helpers (real PyWavelets, float32) in place of
# the restatement's float64 transform, at most 2 of the 12,288 values of any of the 21 images move, by one
# grey level (checked on the CPU when the case was chosen).
E2E_SIZE, E2E_J, E2E_MODEL_SEED = 64, 3, 18
E2E_SEEDS = (60, 61, 62)
E2E_QS = (1.0, 0.99, 0.95, 0.8, 0.5, 0.2, 0.0)   # insertion order; deletion takes them reversed
E2E_LABELS = (0, 3, 7)
E2E_MARGIN = 0.075


def make_e2e():
    """(x [3, 3, S, S] float32 outside [0, 1] so that show() normalises, grad_wams [3, S, S] float64). The images
    are not clipped: a plateau of pixels at exactly 0 or 1 would sit on the grey levels 0.0 and 255.0 of the
    full reconstruction (q = 0), where one float32 ulp of any transform, pywt's included, moves a truncation."""
    xs = []
    for seed in E2E_SEEDS:
        rs = np.random.RandomState(seed)
        yy, xx = np.mgrid[0:E2E_SIZE, 0:E2E_SIZE] / float(E2E_SIZE)
        img = np.stack([0.5 + 0.3 * np.sin(5.0 * xx + c + seed) * np.cos(3.0 * yy - c) for c in range(3)])
        img = img + 0.05 * rs.standard_normal(img.shape)
        xs.append(img * rs.uniform(0.5, 4) - rs.uniform(0, 2))
    return np.stack(xs).astype(np.float32), np.stack([make_map(E2E_SIZE, s) for s in E2E_SEEDS])
