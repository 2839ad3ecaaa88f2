"""Filter banks whose six stored sets differ, the float64 references on them and the case table that the
CPU file (test_filter_banks_ref.py) and the GPU file (test_gpu_filter_banks.py) share.

Every plan keeps ANA = flip(dec), SYN = rec and ADJ = rec (plan_geometry). For an orthogonal wavelet
rec == flip(dec) and hi is the alternating-sign mirror of lo, so a launcher that reads the wrong set, a
kernel that indexes its taps mirrored or one that derives hi from lo computes the right numbers there.
`random_bank` has four unrelated filters; `NAMED` are the table's biorthogonal wavelets, one per length.
"""
import collections
import functools

import numpy as np

from oracle import dwt as D
from tests import epilogue_ref as E
from tests import wavedec_adjoint_ref as R
from wam_amd import filters

MIN_TAP = 0.05


@functools.lru_cache(None)
def random_bank(L, seed):
    """Four independent filters of L taps: uniform(-1, 1), unit l2 norm, float32-representable (the
    plan's fp32 cast is exact), re-drawn until every |tap| >= MIN_TAP so that a dropped or shifted tap
    shows."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(4):
        while True:
            v = rs.uniform(-1, 1, L)
            v = (v / np.sqrt((v * v).sum())).astype(np.float32).astype(np.float64)
            if np.abs(v).min() >= MIN_TAP:
                break
        out.append(tuple(float(t) for t in v))
    return filters.Wavelet("random%d_%d" % (L, seed), *out)


# one table wavelet per even length whose analysis and synthesis sets differ
NAMED = {4: "bior3.1", 6: "bior2.2", 8: "bior3.3", 10: "bior4.4", 12: "rbio3.5", 14: "bior2.6", 16: "bior3.7",
         18: "bior6.8", 20: "bior3.9"}


def get_bank(bank):
    """a CASES bank entry (a tap count -> random_bank(L, L), or a table name) -> filters.Wavelet"""
    return random_bank(bank, bank) if isinstance(bank, int) else filters.get_wavelet(bank)


def taps(w):
    """(dec_lo, dec_hi, rec_lo, rec_hi) float64 arrays: the form oracle.dwt takes in place of a name"""
    return tuple(np.asarray(f, dtype=np.float64) for f in (w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi))


# ------------------------------------------------------------------------------ float64 references
def bands_of(coeffs, ndim):
    """oracle.dwt.*n container [A, {key: band}, ...] -> bands in ptwt order"""
    keys = R.detail_keys(ndim)
    return [coeffs[0]] + [lv[k] for lv in coeffs[1:] for k in keys]


def container_of(bands, ndim):
    keys = R.detail_keys(ndim)
    per = len(keys)
    return [bands[0]] + [dict(zip(keys, bands[1 + per * i:1 + per * (i + 1)])) for i in range((len(bands) - 1) // per)]


def ref_wavedec(x, w, J, mode):
    """x [batch, *shape] -> bands in ptwt order"""
    ndim = np.ndim(x) - 1
    return bands_of(D.wavedecn(x, taps(w), J, mode, ndim), ndim)


def ref_waverec(bands, w, ndim):
    return D.waverecn(container_of([np.asarray(b, dtype=np.float64) for b in bands], ndim), taps(w), ndim)


def ref_adjoint(g, w, J):
    """waverec's VJP: g [batch, *rec_shape] -> bands in ptwt order"""
    ndim = np.ndim(g) - 1
    return bands_of(D.adjointn(g, J, taps(w), ndim), ndim)


def ref_wavedec_adjoint(bands, shape, w, J, mode):
    """wavedec's VJP: bands in ptwt order -> grad_x [batch, *shape]"""
    return R.wavedec_adjoint(bands, tuple(shape), w.dec_lo, w.dec_hi, mode, J)


def band_shapes(shape, L, J):
    return R.band_shapes(tuple(shape), L, J)


def rec_shape(shape, L, J):
    """spatial shape of waverec's output for a plan of `shape`: odd sizes come back one longer"""
    fin = band_shapes(shape, L, J)[-1]
    return tuple(2 * m + 2 - L for m in fin)


def band_offsets(shape, L, J):
    off = [0]
    for s in band_shapes(shape, L, J):
        off.append(off[-1] + int(np.prod(s)))
    return off


def flat_of(bands):
    """bands [batch, *band shape] -> the band-major flat layout of the C ABI"""
    return np.concatenate([np.asarray(b).reshape(-1) for b in bands])


def ref_maps(adj_bands, G, N, C, offsets):
    """maps / band_max of the fused pass from the float64 adjoint's bands [G * N * C, *band shape]"""
    return E.maps_ref(flat_of(adj_bands), G, N, C, offsets)


def f32(a):
    """float32-representable values as float64"""
    return np.asarray(a).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------ the table
GENERIC, NO_ROWS, NO_PLANE = 1, 2, 4
# bank: a tap count L (-> random_bank(L, L)) or a table name; routes: the wam_plan_describe string and wa
# the wam_plan_wavedec_adjoint_route names per level, finest first, both recorded from host-only plans
Case = collections.namedtuple("Case", "ndim shape J bank mode flags routes wa")


def case_id(c):
    return "%dd-%s-J%d-%s-%s-f%d" % (c.ndim, "x".join(map(str, c.shape)), c.J,
                                     c.bank if isinstance(c.bank, str) else "random%d" % c.bank, c.mode, c.flags)


def bank_length(c):
    return c.bank if isinstance(c.bank, int) else len(filters.get_wavelet(c.bank).dec_lo)


def _routes(ana, adj, syn, maps, caps, J):
    lv = lambda r: ",".join([r] * J)
    a, d, s = (r.split("|") for r in (ana, adj, syn))
    return "ana=%s|%s adj=%s|%s syn=%s|%s maps=%s caps=%d" % (a[0], lv(a[1]), d[0], lv(d[1]), s[0], s[1], maps, caps)


def _cases():
    out = []

    def add(ndim, shape, J, Ls, mode, routes, wa, flags=0, named=False):
        """routes: (ana, adj, syn) each 'whole|level', maps, caps; every level of a row has the same route"""
        banks = list(Ls) + ([NAMED[L] for L in Ls if L in NAMED] if named else [])
        for bank in banks:
            out.append(Case(ndim, shape, J, bank, mode, flags, _routes(*routes, J), (wa,) * J))

    plane = ("plane|rows", "plane|rows", "plane|colstrip", "plane", 7)
    rows = ("none|rows", "none|rows", "none|colstrip", "rows", 3)
    rows_no_plane = rows[:4] + (2,)
    colstrip = ("none|colstrip", "none|colstrip", "none|colstrip", "none", 0)
    axis = ("none|axis", "none|axis", "none|axis", "none", 0)
    tile1 = ("tile1|axis", "tile1|axis", "tile1|axis", "none", 1)
    tile3 = ("none|tile3", "none|tile3", "none|tile3", "none", 0)
    haar3 = ("haar3|tile3", "haar3|tile3", "haar3|tile3", "none", 1)
    # 2D
    add(2, (36, 44), 2, [2, 4, 6, 8], "reflect", plane, "fold2d", named=True)
    add(2, (36, 44), 2, [12, 16, 20], "reflect", rows, "fold2d", named=True)
    add(2, (36, 44), 2, [10, 14, 18], "reflect", colstrip, "fold2d", named=True)
    add(2, (37, 50), 2, [10, 14, 18], "zero", colstrip, "fold2d")                   # odd height
    add(2, (37, 50), 2, [2, 4, 6, 8, 12, 16, 20], "symmetric", rows_no_plane, "fold2d", NO_PLANE)
    add(2, (33, 40), 2, [8], "constant", colstrip, "fold2d", NO_ROWS)               # colstrip with a short filter
    add(2, (40, 520), 1, [6], "periodic", ("none|colstrip", "none|colstrip", "plane|colstrip", "none", 0), "fold2d")
    add(2, (30, 26), 2, [4], "zero", ("none|rows", "none|rows", "plane|colstrip", "rows", 2), "fold2d")
    add(2, (64, 64), 2, [22], "reflect", axis, "axis")
    add(2, (36, 44), 2, [8], "reflect", axis, "axis", GENERIC)
    # n <= pad: several reflections; the wavedec adjoint takes the per-axis route inside a fused plan
    add(2, (6, 30), 2, [8], "reflect", ("none|rows", "none|rows", "plane|colstrip", "rows", 2), "axis")
    # 1D: boundary tiles; reflect / symmetric alternating over the lengths
    for i, L in enumerate(range(2, 21, 2)):
        add(1, (1000,), 3, [L], ("reflect", "symmetric")[i % 2], tile1, "axis", named=True)
    add(1, (33000,), 3, [12], "constant", tile1, "axis")                            # interior tiles
    add(1, (33000,), 3, [6], "zero", tile1, "axis")
    add(1, (300,), 2, [8], "periodic", ("none|axis", "tile1|axis", "none|axis", "none", 0), "axis")
    add(1, (300,), 2, [22], "reflect", axis, "axis")
    # 3D
    add(3, (9, 10, 11), 2, [2, 4, 6, 8], "symmetric", tile3, "axis", named=True)
    add(3, (16, 12, 8), 2, [2], "reflect", haar3, "axis")                           # a 2-tap bank that is not Haar
    add(3, (8, 8, 8), 1, [2], "zero", haar3, "axis")
    add(3, (12, 10, 9), 1, [6], "periodic", tile3, "axis")
    add(3, (9, 10, 11), 1, [10], "reflect", axis, "axis")
    return out


CASES = _cases()
