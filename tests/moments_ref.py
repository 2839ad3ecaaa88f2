"""Float64 restatement of the 'smooth_sq' / 'vargrad' methods on the CPU, from
existing pieces of oracle/wam_ref.py only: legacy_noise_stream, single_pass_2d / 1d / 3d, mosaic_2d,
frame_geometry (refactor_3d through single_pass_3d). Per noise sample s the map v_s is what the
reference's SmoothGrad adds; then, in sample order,

    S += v_s,  Q += v_s * v_s   (float64),   mean = S / n,  smooth_sq = Q / n,
    vargrad = max(Q / n - mean * mean, 0)          (the population variance)

The 3D moments use this plain mean, not the in-loop averaging of the reference's 3D 'smooth'.
Shared inputs of tests/test_moments_ref.py (CPU) and tests/test_gpu_moments.py live here, and every
reference is computed once per process (lru_cache) and handed out read-only.
"""
import functools

import numpy as np
import torch

import testmodels
from oracle import wam_ref

N_SAMPLES = 6
SEED = 42
LABELS_2D = [1, 3]
# the two 2D inputs: torch.rand (seed 1), stdev_spread 0.25, native frame
CASES_2D = {"haar_J2_32": dict(wavelet="haar", J=2, size=32), "db4_J3_64": dict(wavelet="db4", J=3, size=64)}
SPREAD_2D = 0.25
KW_1D = dict(wavelet="db6", J=2, mode="reflect", sample_rate=16000, stdev_spread=0.01)
LEN_1D, LABELS_1D = 4096, [1, 2]
KW_3D = dict(wavelet="haar", J=2, mode="symmetric", stdev_spread=0.05)
SIZE_3D, LABELS_3D = 16, [1, 2]


def moments(maps):
    """maps: the per-sample arrays v_s in sample order -> dict(S, Q, mean, smooth_sq, vargrad), float64."""
    n = len(maps)
    S = np.zeros(np.shape(maps[0]), dtype=np.float64)
    Q = np.zeros_like(S)
    for v in maps:
        v = np.asarray(v, dtype=np.float64)
        S = S + v
        Q = Q + v * v
    mean = S / n
    out = dict(S=S, Q=Q, mean=mean, smooth_sq=Q / n, vargrad=np.maximum(Q / n - mean * mean, 0.0))
    for a in out.values():
        a.setflags(write=False)
    return out


def inputs_2d(name):
    torch.manual_seed(1)
    s = CASES_2D[name]["size"]
    return torch.rand(2, 3, s, s)


def sample_maps_2d(name, stdev_spread=SPREAD_2D, n_samples=N_SAMPLES):
    """[n_samples, N, H, W] float64: the normalised native-frame mosaic of every noise sample."""
    c = CASES_2D[name]
    x = inputs_2d(name)
    model = testmodels.TinySmooth2D()
    H, W = x.shape[2], x.shape[3]
    out = []
    for _, noisy in wam_ref.legacy_noise_stream(x, n_samples, stdev_spread, SEED):
        _, g = wam_ref.single_pass_2d(model, noisy, LABELS_2D, c["wavelet"], c["J"], "reflect")
        canvas, base = wam_ref.frame_geometry("native", H, W, g[-1][0].shape[-1])
        out.append(wam_ref.mosaic_2d(g, True, canvas, base))
    return np.stack(out)


@functools.lru_cache(None)
def ref_2d(name):
    v = sample_maps_2d(name)
    v.setflags(write=False)
    return dict(moments(list(v)), maps=v)


def inputs_1d():
    return torch.tensor(np.random.RandomState(5).standard_normal((2, LEN_1D)).astype(np.float32))


@functools.lru_cache(None)
def ref_1d():
    """moments of the flattened (melspec gradient, band gradients...) vector per sample, split back:
    dict of kind -> (mel, [bands])."""
    kw = KW_1D
    x = inputs_1d()
    model = testmodels.TinyAudio()
    per, shapes = [], None
    for _, noisy in wam_ref.legacy_noise_stream(x, N_SAMPLES, kw["stdev_spread"], SEED):
        m, g = wam_ref.single_pass_1d(model, noisy, LABELS_1D, kw["wavelet"], kw["J"], kw["mode"], 1024,
                                      kw["sample_rate"], 128)
        parts = [m] + list(g)
        shapes = [p.shape for p in parts]
        per.append(np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]))
    mo = moments(per)
    cuts = np.cumsum([int(np.prod(s)) for s in shapes])[:-1]
    out = {}
    for k, a in mo.items():
        parts = [p.reshape(s) for p, s in zip(np.split(a, cuts), shapes)]
        out[k] = (parts[0], parts[1:])
    out["maps"] = np.stack(per)
    return out


def inputs_3d():
    rs = np.random.RandomState(3)
    return torch.tensor((rs.standard_normal((2, 1, SIZE_3D, SIZE_3D, SIZE_3D)) > 0).astype(np.float32))


@functools.lru_cache(None)
def ref_3d():
    kw = KW_3D
    x = inputs_3d()
    model = testmodels.TinyVoxel()
    per = [wam_ref.single_pass_3d(model, noisy, LABELS_3D, kw["wavelet"], kw["J"], kw["mode"], SIZE_3D)
           for _, noisy in wam_ref.legacy_noise_stream(x, N_SAMPLES, kw["stdev_spread"], SEED, item_slice=0)]
    v = np.stack(per)
    v.setflags(write=False)
    return dict(moments(per), maps=v)
