"""The references and the case table of tests/filter_banks.py, checked without a device:

1. oracle.dwt with a 4-tuple bank equals PyWavelets on biorthogonal and random banks (tests/golden/pywt_bior.npz,
   written by tests/golden/make_pywt_bior_fixtures.py), to the bar of test_numpy_oracle_vs_pywt: every bank
   through all five modes in 1D; in 2D one shape and one mode per bank, both shapes meeting every mode over the
   banks (the float64 answers do not compress: more would not fit the size limit of a committed file);
2. the dot-product identities of both adjoint references hold in float64 on every random bank;
3. the references have teeth: with the filter sets exchanged (dec <-> rec, a filter reversed, hi derived from
   lo) every band moves by more than 1000 times the bar the GPU tests hold the kernels to;
4. the table reaches every kernel route with every tap count that route supports, on host-only plans, and
   every row's routes are the recorded ones.
"""
import ctypes
import re

import numpy as np
import pytest

from tests import filter_banks as F
from tests.helpers import npz
from tests.test_wavedec_adjoint_host import host_plan, lib

LENGTHS = list(range(2, 23, 2))
ANA_BAR, SYN_BAR, WA_BAR = 2e-6, 8e-6, 8e-6    # the GPU bars, each times max(1, max|ref|)


# ------------------------------------------------------------------------------ 1. pywt
def _fixture_cases():
    d = npz("pywt_bior.npz")
    dims, data = d["dims"], d["data"]
    di = off = 0
    for name, mode, J, shape in d["cases"]:
        shape = tuple(int(s) for s in str(shape).split("x"))
        ndim, J = len(shape), int(J)
        nb = 1 + J * ((1 << ndim) - 1)
        arrays = []
        for _ in range(2 * nb + 2):
            s = tuple(int(v) for v in dims[di:di + ndim + 1])
            di += ndim + 1
            arrays.append(data[off:off + int(np.prod(s))].reshape(s))
            off += int(np.prod(s))
        yield str(name), str(mode), J, shape, arrays[0], arrays[1:1 + nb], arrays[1 + nb:1 + 2 * nb], arrays[-1]
    assert di == len(dims) and off == len(data)


def _fixture_bank(name):
    return F.filters.Wavelet(name, *[tuple(map(float, f)) for f in npz("pywt_bior.npz")["bank_" + name]])


def test_random_bank_reproduces_the_stored_taps():
    d = npz("pywt_bior.npz")
    for L in LENGTHS:
        w = F.random_bank(L, L)
        got = np.array([w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi])
        assert np.array_equal(got, d["bank_random%d" % L]), L
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
        assert np.abs(got).min() >= F.MIN_TAP and np.allclose((got * got).sum(axis=1), 1.0, atol=1e-6)
    for name in F.NAMED.values():  # the fixture's table wavelets are the package's
        assert np.array_equal(np.array(F.taps(F.filters.get_wavelet(name))), d["bank_" + name]), name


def test_named_banks_have_differing_sets():
    for L, name in F.NAMED.items():
        dl, dh, rl, rh = F.taps(F.filters.get_wavelet(name))
        assert len(dl) == L
        assert not np.allclose(rl, dl[::-1]) and not np.allclose(rh, dh[::-1]), name


def test_oracle_matches_pywt_on_non_orthogonal_banks():
    seen = set()
    worst = 0.0
    for name, mode, J, shape, x, cs, rs, rrec in _fixture_cases():
        w = _fixture_bank(name)
        ndim = len(shape)
        seen.add((name, ndim, mode))
        got = F.ref_wavedec(x, w, J, mode)
        assert len(got) == len(cs)
        for b, (g, r) in enumerate(zip(got, cs)):
            assert g.shape == r.shape, (name, mode, shape, b)
            worst = max(worst, np.abs(g - r).max())
            assert np.abs(g - r).max() < 1e-10, (name, mode, shape, b)
        rec = F.ref_waverec(rs, w, ndim)
        assert all(a <= b for a, b in zip(rec.shape, rrec.shape)), (rec.shape, rrec.shape)
        ref = rrec[tuple(slice(0, s) for s in rec.shape)]  # pywt's output cropped to the oracle's shape
        worst = max(worst, np.abs(rec - ref).max())
        assert np.abs(rec - ref).max() < 1e-10, (name, mode, shape)
    print("oracle vs pywt: worst %.3g" % worst)
    names = list(F.NAMED.values()) + ["random%d" % L for L in LENGTHS]
    for name in names:  # every bank through every mode in 1D and through 2D
        assert {m for n, k, m in seen if n == name and k == 1} == set(F.D.MODES), name
        assert any(n == name and k == 2 for n, k, m in seen), name
    assert {m for n, k, m in seen if k == 2} == set(F.D.MODES) and any(k == 3 for n, k, m in seen)


# ------------------------------------------------------------------------------ 2. identities
IDENTITY_SHAPES = [((37,), 2), ((13, 10), 2), ((7, 6, 5), 1)]


def _inputs(rs, shape, L, J, batch=2):
    x = rs.standard_normal((batch,) + shape)
    c = [rs.standard_normal((batch,) + s) for s in F.band_shapes(shape, L, J)]
    g = rs.standard_normal((batch,) + F.rec_shape(shape, L, J))
    return x, c, g


def _dot(a, b):
    return sum(float((u * v).sum()) for u, v in zip(a, b))


@pytest.mark.parametrize("L", LENGTHS)
def test_dot_product_identities(L):
    w = F.random_bank(L, L)
    rs = np.random.RandomState(100 + L)
    for shape, J in IDENTITY_SHAPES:
        for mode in F.D.MODES:
            x, c, g = _inputs(rs, shape, L, J)
            rec = F.ref_waverec(c, w, len(shape))
            assert rec.shape == g.shape
            lhs, rhs = _dot([rec], [g]), _dot(c, F.ref_adjoint(g, w, J))
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (shape, lhs, rhs)
            lhs = _dot(F.ref_wavedec(x, w, J, mode), c)
            rhs = _dot([x], [F.ref_wavedec_adjoint(c, shape, w, J, mode)])
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (shape, mode, lhs, rhs)


# ------------------------------------------------------------------------------ 3. teeth
def _mirror(lo):
    """the alternating-sign mirror that gives an orthogonal wavelet's high-pass from its low-pass"""
    return tuple(((-1.0) ** k) * v for k, v in enumerate(lo[::-1]))


def _exchanges(w):
    W = F.filters.Wavelet
    return {
        # a launcher that reads the synthesis sets for the analysis and the other way round
        "dec<->rec": W("x", w.rec_lo, w.rec_hi, w.dec_lo, w.dec_hi),
        # the same without the flip that ANA = flip(dec) carries
        "dec<->flip(rec)": W("x", w.rec_lo[::-1], w.rec_hi[::-1], w.dec_lo[::-1], w.dec_hi[::-1]),
        # a kernel that indexes its taps mirrored
        "reversed": W("x", w.dec_lo[::-1], w.dec_hi[::-1], w.rec_lo[::-1], w.rec_hi[::-1]),
        # a kernel that derives the high-pass from the low-pass
        "hi=mirror(lo)": W("x", w.dec_lo, _mirror(w.dec_lo), w.rec_lo, _mirror(w.rec_lo)),
    }


def _all_four(w, x, c, g, shape, J, mode):
    return {"ana": F.ref_wavedec(x, w, J, mode), "adj": F.ref_adjoint(g, w, J),
            "syn": [F.ref_waverec(c, w, len(shape))], "wa": [F.ref_wavedec_adjoint(c, shape, w, J, mode)]}


@pytest.mark.parametrize("L", LENGTHS)
def test_exchanged_sets_move_every_band(L):
    """What a kernel with such a mistake would compute lies more than 1000 bars from the reference: on every
    band of the analysis and of the adjoint, on the synthesis and on the wavedec adjoint. (The approximation
    band never passes a high-pass filter, so the last exchange is held to the detail bands.)"""
    w = F.random_bank(L, L)
    rs = np.random.RandomState(200 + L)
    bars = {"ana": ANA_BAR, "adj": SYN_BAR, "syn": SYN_BAR, "wa": WA_BAR}
    for shape, J in IDENTITY_SHAPES:
        x, c, g = _inputs(rs, shape, L, J)
        ref = _all_four(w, x, c, g, shape, J, "reflect")
        for what, v in _exchanges(w).items():
            got = _all_four(v, x, c, g, shape, J, "reflect")
            for k in ref:
                for b, (r, t) in enumerate(zip(ref[k], got[k])):
                    if what == "hi=mirror(lo)" and k in ("ana", "adj") and b == 0:
                        assert np.array_equal(t, r)
                        continue
                    ratio = np.abs(t - r).max() / (bars[k] * max(1.0, np.abs(r).max()))
                    assert ratio > 1000, (L, shape, what, k, b, ratio)


# ------------------------------------------------------------------------------ 4. routes
def _describe(c):
    h = host_plan(c.ndim, c.shape, c.J, F.get_bank(c.bank), c.mode, c.flags)
    try:
        buf = ctypes.create_string_buffer(512)
        assert lib.wam_plan_describe(h, buf, len(buf)) == 0
        wa = [("axis", "fold2d")[lib.wam_plan_wavedec_adjoint_route(h, l)] for l in range(c.J)]
        return buf.value.decode(), wa
    finally:
        lib.wam_plan_destroy(h)


@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_case_routes_are_the_recorded_ones(case):
    assert _describe(case) == (case.routes, list(case.wa))


def test_table_reaches_every_route_with_every_tap_count():
    pat = re.compile(r"ana=(\w+)\|([\w,]+) adj=(\w+)\|([\w,]+) syn=(\w+)\|(\w+) maps=(\w+) caps=(\d+)")
    seen = set()
    for c in F.CASES:
        L = F.bank_length(c)
        ana_w, ana_l, adj_w, adj_l, syn_w, syn_l, maps, _ = pat.fullmatch(c.routes).groups()
        for kind, whole, levels in (("ana", ana_w, ana_l), ("adj", adj_w, adj_l), ("syn", syn_w, syn_l)):
            seen.add((kind, "whole", whole, L))
            if whole == "none":  # the level routes run only without a whole-transform kernel
                seen.update((kind, "level", r, L) for r in levels.split(","))
        seen.add(("maps", "whole", maps, L))
        seen.update(("wa", "level", r, L) for r in c.wa)
    # every route value occurs in the transforms that have it ...
    pairs = [(k, "whole", r) for k in ("ana", "adj", "syn") for r in ("plane", "tile1", "haar3")]
    pairs += [(k, "level", r) for k in ("ana", "adj") for r in ("rows", "colstrip", "tile3", "axis")]
    pairs += [("syn", "level", r) for r in ("colstrip", "tile3", "axis")]
    pairs += [("maps", "whole", "plane"), ("maps", "whole", "rows"), ("wa", "level", "fold2d"), ("wa", "level", "axis")]
    missing = [p for p in pairs if p not in {s[:3] for s in seen}]
    assert not missing, missing
    # ... and every route runs with every tap count it is instantiated for
    short, even = [2, 4, 6, 8], list(range(2, 21, 2))
    want = {"plane": short, "tile3": short, "rows": short + [12, 16, 20], "colstrip": even, "tile1": even,
            "haar3": [2], "axis": [22], "fold2d": even}
    missing = [(r, L) for r, Ls in want.items() for L in Ls if (r, L) not in {s[2:] for s in seen}]
    assert not missing, missing
    # the column-strip analysis has instantiations of its own where the row kernel has none
    missing = [(k, L) for k in ("ana", "adj") for L in (10, 14, 18) if (k, "level", "colstrip", L) not in seen]
    assert not missing, missing
    # every named wavelet runs wherever a row is marked for them, and differs from the random bank of its length
    assert {c.bank for c in F.CASES if isinstance(c.bank, str)} == set(F.NAMED.values())
