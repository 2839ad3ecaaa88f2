"""Generate the known answers that pin oracle.dwt to PyWavelets on filter banks whose analysis and
synthesis sets differ (tests/test_filter_banks_ref.py). Run with the interpreter that
make_pywt_fixtures.py names; it needs numpy and pywt only:

    python3.9 tests/golden/make_pywt_bior_fixtures.py

Banks: the biorthogonal table wavelets of tests/filter_banks.py NAMED, and random banks of 2..22 taps
given to pywt as ``pywt.Wavelet(name, filter_bank=[...])``. The random banks are built here by the rule
of tests/filter_banks.random_bank, restated so that this file needs nothing of the package; the taps are
stored (``bank_<name>``, rows dec_lo, dec_hi, rec_lo, rec_hi) and the test holds random_bank to them.

Cases (batch 1): row i of ``cases`` = bank, mode, J, shape; its arrays lie one after the other in ``data``
with their shapes in ``dims`` (1 + ndim numbers each), in the order input, pywt.wavedec* bands in ptwt
order, random coefficients of the same shapes, pywt.waverec* of those:

* 1D (37,) J=2 and (64,) J=3: every bank, all five modes;
* 2D (24, 24) and (29, 35), J=2: every bank. The answers are full-entropy float64 and do not compress;
  both shapes in two modes for every bank would take about 2 MB. So bank number i gets one shape
  (even i: (24, 24), odd i: (29, 35)) and one mode, the five modes taken in turn, reflect first: over the
  banks both shapes meet every mode. The transform is separable, and the 1D cases carry every bank
  through every mode;
* 3D (13, 11, 10) J=1: random4 reflect and bior2.2 zero (60 KB a case).

Inputs and random coefficients are multiples of 1/16 in [-4, 4] (they compress; the answers are what
takes the room). Output: tests/golden/pywt_bior.npz.
"""
import os

import numpy as np
import pywt

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ["reflect", "zero", "symmetric", "constant", "periodic"]
NAMED = ["bior3.1", "bior2.2", "bior3.3", "bior4.4", "rbio3.5", "bior2.6", "bior3.7", "bior6.8", "bior3.9"]
KEYS3 = ["aad", "ada", "add", "daa", "dad", "dda", "ddd"]


def random_bank(L, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(4):
        while True:
            v = rs.uniform(-1, 1, L)
            v = (v / np.sqrt((v * v).sum())).astype(np.float32).astype(np.float64)
            if np.abs(v).min() >= 0.05:
                break
        out.append(v)
    return np.stack(out)


def banks():
    out = [(name, pywt.Wavelet(name)) for name in NAMED]
    for L in range(2, 23, 2):
        name = "random%d" % L
        out.append((name, pywt.Wavelet(name, filter_bank=[list(f) for f in random_bank(L, L)])))
    return out


def draw(rs, shape):
    return rs.randint(-64, 65, size=shape) / 16.0


def flat(cs, ndim):
    """pywt container -> bands in ptwt order (2D: pywt's (cH, cV, cD) are the keys da, ad, dd)"""
    if ndim == 1:
        return list(cs)
    if ndim == 2:
        return [cs[0]] + [b for lv in cs[1:] for b in lv]
    return [cs[0]] + [lv[k] for lv in cs[1:] for k in KEYS3]


def container(bands, ndim):
    if ndim == 1:
        return list(bands)
    if ndim == 2:
        return [bands[0]] + [tuple(bands[1 + 3 * i:4 + 3 * i]) for i in range((len(bands) - 1) // 3)]
    return [bands[0]] + [dict(zip(KEYS3, bands[1 + 7 * i:8 + 7 * i])) for i in range((len(bands) - 1) // 7)]


def main():
    rs = np.random.RandomState(20250301)
    store, meta, dims, data = {}, [], [], []

    def case(name, w, shape, J, mode):
        ndim = len(shape)
        axes = tuple(range(-ndim, 0))
        dec = {1: lambda x: pywt.wavedec(x, w, mode=mode, level=J, axis=-1),
               2: lambda x: pywt.wavedec2(x, w, mode=mode, level=J, axes=axes),
               3: lambda x: pywt.wavedecn(x, w, mode=mode, level=J, axes=axes)}[ndim]
        rec = {1: lambda c: pywt.waverec(c, w, mode=mode, axis=-1),
               2: lambda c: pywt.waverec2(c, w, mode=mode, axes=axes),
               3: lambda c: pywt.waverecn(c, w, mode=mode, axes=axes)}[ndim]
        x = draw(rs, (1,) + shape)
        bands = flat(dec(x), ndim)
        rnd = [draw(rs, b.shape) for b in bands]
        arrays = [x] + [np.asarray(b) for b in bands] + rnd + [np.asarray(rec(container(rnd, ndim)))]
        meta.append([name, mode, str(J), "x".join(map(str, shape))])
        for a in arrays:
            assert a.ndim == ndim + 1
            dims.extend(a.shape)
            data.append(a.reshape(-1))

    for i, (name, w) in enumerate(banks()):
        store["bank_" + name] = np.array(w.filter_bank, dtype=np.float64)
        for mode in MODES:
            case(name, w, (37,), 2, mode)
            case(name, w, (64,), 3, mode)
        case(name, w, ((24, 24), (29, 35))[i % 2], 2, MODES[i % 5])
        if name == "random4":
            case(name, w, (13, 11, 10), 1, "reflect")
        if name == "bior2.2":
            case(name, w, (13, 11, 10), 1, "zero")
    path = os.path.join(HERE, "pywt_bior.npz")
    # one entry per kind, not per array: a zip member costs more than a 1D case holds
    np.savez_compressed(path, cases=np.array(meta), dims=np.array(dims, dtype=np.int32), data=np.concatenate(data),
                        **store)
    print("wrote", path, len(meta), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
