"""float64 numpy statement of the wavedec adjoint (the backward pass of ``wavedec*`` with respect to the
analysed signal), written from its formula and independent of the kernels and of autograd.

Per axis of one level, with n input samples, L taps, p = (2L-3)//2, padl = p, padr = p + n%2,
m = (n + padl + padr - L)//2 + 1 and T = n + padl + padr:

    y[t]  = sum_j f_lo[t-2j] glo[j] + f_hi[t-2j] ghi[j]            0 <= t < T, 0 <= t-2j < L
    gx[i] = sum of y[t] over the t with ext(t - padl) == i          0 <= i < n

f_lo / f_hi are the reversed decomposition filters (what the analysis correlates with) and ext is the
boundary extension. Levels run coarsest to finest; a level's result has exactly that level's input
shape. tests/test_wavedec_adjoint_ref.py pins this file to autograd through oracle.ptwt_torch.
"""
import itertools

import numpy as np

MODES = ("zero", "constant", "symmetric", "reflect", "periodic")

# the issue's case list: (ndim, wavelet, shape, levels)
CASES = [
    (1, "haar", (2,), 1), (1, "haar", (8,), 2), (1, "db2", (5,), 2), (1, "db6", (7,), 2), (1, "db4", (37,), 3),
    (1, "bior2.2", (10,), 2),
    (2, "db4", (3, 4), 2), (2, "db4", (9, 11), 2), (2, "sym8", (20, 23), 2), (2, "bior2.2", (10, 12), 2),
    (3, "db2", (6, 7, 5), 1), (3, "sym8", (5, 6, 4), 1),
]


def case_id(case):
    return "%dd-%s-%s-J%d" % (case[0], case[1], "x".join(map(str, case[2])), case[3])


def ext(i, n, mode):
    """Source index of extended position i (-1: zero padding), any number of wraps."""
    if 0 <= i < n:
        return i
    if mode == "zero":
        return -1
    if mode == "constant":
        return 0 if i < 0 else n - 1
    if mode == "periodic":
        return i % n
    if mode == "reflect":
        if n == 1:
            return 0
        r = i % (2 * n - 2)
        return 2 * n - 2 - r if r >= n else r
    if mode == "symmetric":
        r = i % (2 * n)
        return 2 * n - 1 - r if r >= n else r
    raise ValueError(mode)


def sizes(n, L):
    p = (2 * L - 3) // 2
    padl, padr = p, p + n % 2
    m = (n + padl + padr - L) // 2 + 1
    return padl, padr, m


def fold_matrices(n, f_lo, f_hi, mode):
    """(M_lo, M_hi), each [n, m]: gx = M_lo @ glo + M_hi @ ghi along the axis."""
    L = len(f_lo)
    padl, padr, m = sizes(n, L)
    T = n + padl + padr
    assert T == 2 * m - 2 + L
    M_lo = np.zeros((n, m))
    M_hi = np.zeros((n, m))
    for t in range(T):
        i = ext(t - padl, n, mode)
        if i < 0:
            continue
        for j in range(m):
            k = t - 2 * j
            if 0 <= k < L:
                M_lo[i, j] += f_lo[k]
                M_hi[i, j] += f_hi[k]
    return M_lo, M_hi


def detail_keys(ndim):
    """Detail band order of one level ('a' / 'd' per axis, first letter = first axis), ptwt's."""
    if ndim == 2:
        return ["da", "ad", "dd"]
    return ["".join(t) for t in itertools.product("ad", repeat=ndim)][1:]


def level_shapes(shape, L, levels):
    """Input shape of every level, finest first, and the band shape of every level."""
    lin, lout = [], []
    cur = tuple(shape)
    for _ in range(levels):
        lin.append(cur)
        cur = tuple(sizes(n, L)[2] for n in cur)
        lout.append(cur)
    return lin, lout


def band_shapes(shape, L, levels):
    """Band shapes in ptwt order [A_J, details_J ..., details_1]."""
    ndim = len(shape)
    _, lout = level_shapes(shape, L, levels)
    out = [lout[-1]]
    for l in range(levels - 1, -1, -1):
        out += [lout[l]] * ((1 << ndim) - 1)
    return out


def oracle_bands(coeffs, ndim):
    """oracle.ptwt_torch container -> list of band tensors in ptwt order."""
    if ndim == 1:
        return list(coeffs)
    if ndim == 2:
        return [coeffs[0]] + [t for lv in coeffs[1:] for t in lv]
    return [coeffs[0]] + [lv[k] for lv in coeffs[1:] for k in detail_keys(3)]


def oracle_gradient(x, band_grads, wavelet, mode, levels, dtype):
    """d <wavedec(x), band_grads> / dx by autograd through oracle.ptwt_torch, computed in `dtype`
    (x: [batch, *shape], band_grads: arrays in ptwt order); returned as a float64 array."""
    import torch

    from oracle import ptwt_torch as P
    ndim = x.ndim - 1
    dec = {1: P.wavedec, 2: P.wavedec2, 3: P.wavedec3}[ndim]
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    bands = oracle_bands(dec(xt, wavelet, mode=mode, level=levels), ndim)
    assert [tuple(b.shape) for b in bands] == [tuple(np.shape(g)) for g in band_grads]
    loss = sum((b * torch.tensor(np.asarray(g), dtype=dtype)).sum() for b, g in zip(bands, band_grads))
    (gx,) = torch.autograd.grad(loss, xt)
    return gx.double().numpy()


def case_inputs(case, batch=2, seed=0):
    """(x, band_grads) of a case: float32-representable values as float64 arrays."""
    from oracle import dwt as D
    ndim, wavelet, shape, levels = case
    L = len(D.filter_bank(wavelet)[0])
    rs = np.random.RandomState(seed + 7 * ndim + sum(shape))
    x = rs.standard_normal((batch,) + tuple(shape)).astype(np.float32).astype(np.float64)
    grads = [rs.standard_normal((batch,) + tuple(s)).astype(np.float32).astype(np.float64)
             for s in band_shapes(shape, L, levels)]
    return x, grads


def _apply(M, g, axis):
    return np.moveaxis(np.tensordot(M, g, axes=([1], [axis])), 0, axis)


def wavedec_adjoint(band_grads, shape, dec_lo, dec_hi, mode, levels):
    """band_grads: arrays [batch, *band shape] in ptwt order -> grad_x [batch, *shape] (float64)."""
    ndim = len(shape)
    f_lo = np.asarray(dec_lo, dtype=np.float64)[::-1]
    f_hi = np.asarray(dec_hi, dtype=np.float64)[::-1]
    lin, _ = level_shapes(shape, len(f_lo), levels)
    keys = detail_keys(ndim)
    per = len(keys)
    approx = np.asarray(band_grads[0], dtype=np.float64)
    for c in range(levels):
        l = levels - 1 - c
        parts = {"a" * ndim: approx}
        for k, key in enumerate(keys):
            parts[key] = np.asarray(band_grads[1 + c * per + k], dtype=np.float64)
        for ax in range(ndim - 1, -1, -1):  # the axes are separable: last axis first
            M_lo, M_hi = fold_matrices(lin[l][ax], f_lo, f_hi, mode)
            merged = {}
            for key, g in parts.items():
                if key[ax] != "a":
                    continue
                hi = parts[key[:ax] + "d" + key[ax + 1:]]
                merged[key] = _apply(M_lo, g, 1 + ax) + _apply(M_hi, hi, 1 + ax)
            parts = merged
        approx = parts["a" * ndim]
        assert approx.shape[1:] == lin[l]
    return approx
