"""The three Eval1DWAM kernels (wam_amd/csrc/evaluate1d.hip) at c3's evaluation geometry -- haar J=5,
8 clips of 80,000 samples, n_iter = 64, so 520 model rows -- and one end-to-end
``deletion(x, y, 'wavelet', 64)`` against the numpy restatement of the reference's per-clip CPU loop
(tests/eval1d_ref.py) on the host's cores.

Per kernel: the time per call from HIP events over enough repetitions to fill --window seconds,
after a warm-up; the algorithmic bytes from the shapes (every input read once, every output written
once); achieved bytes/s and its share of the 8 TB/s HBM peak. These are elementwise and reduction
passes next to a model forward: the shares show what fusing them into the neighbouring kernels
(the mask into the synthesis load, the normalisation into k_mel_fwd's load) would still buy.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8e12


def timed(fn, window):
    """ms per call: warm up, size the repetition count to `window` seconds, time with device events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    iters = max(10, int(window * 1e3 / max(s.elapsed_time(e), 1e-3)))
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, iters


def row(name, ms, iters, nbytes):
    rate = nbytes / (ms * 1e-3)
    print("%-22s %9.1f us x %6d  %8.1f MB  %7.0f GB/s  %5.1f %% of 8 TB/s"
          % (name, 1e3 * ms, iters, nbytes / 1e6, rate / 1e9, 100 * rate / HBM_PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--samples", type=int, default=80000)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--n-iter", type=int, default=64)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per kernel")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the CPU restatement")
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_eval1d needs a HIP device"
    import testmodels
    from wam_amd._lib import check, lib, ptr, stream_of
    from wam_amd.evaluation import Eval1DWAM, coeff_slot_map
    from wam_amd.plan import get_plan

    dev = torch.device("cuda", 0)
    n, T, J, n_iter = a.clips, a.samples, a.levels, a.n_iter
    M = n_iter + 1
    plan = get_plan(1, (T,), J, "haar", "reflect", dev)
    K = plan.coeff_numel
    pos = torch.as_tensor(coeff_slot_map(T, J, [s[0] for s in plan.band_shapes])).to(dev)
    x = testmodels.audio_clips(n, T).to(dev)
    coeffs = plan.wavedec(x)
    rank = torch.stack([torch.randperm(K, device=dev) for _ in range(n)]).to(torch.int32).contiguous()
    masked = torch.empty(n * M * K, dtype=torch.float32, device=dev)
    st = stream_of(dev)
    print("geometry: %d clips x %d samples, haar J=%d, n_iter=%d -> %d rows, %d coefficients per clip"
          % (n, T, J, n_iter, n * M, K))
    print("%-22s %12s   %8s  %10s  %11s  %s" % ("kernel", "time / call", "reps", "alg. bytes", "achieved", "share"))

    ms, it = timed(lambda: check(lib.wam_rank_mask_coeffs(plan.handle, n, ptr(coeffs), ptr(rank), K, ptr(pos), n_iter,
                                                          int(K / n_iter), 1, ptr(masked), st)), a.window)
    row("wam_rank_mask_coeffs", ms, it, 4.0 * (n * K + n * K + K + n * M * K))

    rec = plan.waverec(masked, n * M)[0].view(n * M, -1).contiguous()
    out = torch.empty_like(rec)
    flags = torch.empty(n * M, dtype=torch.int32, device=dev)
    ms, it = timed(lambda: check(lib.wam_peak_normalize(n * M, rec.shape[1], ptr(rec), ptr(out), ptr(flags), 0, st)),
                   a.window)
    row("wam_peak_normalize", ms, it, 8.0 * rec.numel())

    F = T // 512 + 1
    mel = torch.randn(n, F * 128, device=dev)
    mrank = torch.stack([torch.randperm(F * 128, device=dev) for _ in range(n)]).to(torch.int32).contiguous()
    mout = torch.empty(n * M * F * 128, dtype=torch.float32, device=dev)
    ms, it = timed(lambda: check(lib.wam_rank_mask_rows(n, F * 128, ptr(mel), ptr(mrank), n_iter,
                                                        int(F * 128 / n_iter), 1, ptr(mout), st)), a.window)
    row("wam_rank_mask_rows", ms, it, 4.0 * (2 * n * F * 128 + n * M * F * 128))
    if a.skip_end_to_end:
        return

    # ---- end to end: one deletion call, the device class vs the per-clip CPU loop, same grad_wams
    from tests import eval1d_ref as R
    y = list(range(n))
    kw = dict(wavelet="haar", J=J, n_mels=128, n_fft=1024, sample_rate=16000, n_samples=2)
    ev = Eval1DWAM(testmodels.FtEx(seed=0).to(dev), **kw, tie_order="numpy")
    ev.grad_wams = ev.gradwam(x, y)
    ev.deletion(x, y, "wavelet", n_iter)           # warm-up: plans, tables, MIOpen's algorithm search
    torch.cuda.synchronize()
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        scores = ev.deletion(x, y, "wavelet", n_iter)
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / reps
    torch.set_num_threads(a.threads)
    cfg = dict(wavelet="haar", J=J, n_fft=1024, sample_rate=16000, n_mels=128)
    model = testmodels.FtEx(seed=0)
    xc = x.cpu().numpy()
    t0 = time.perf_counter()
    ref_scores, ref_curves, _ = R.evaluate_auc(model, xc, y, ev.grad_wams, "deletion", "wavelet", n_iter, cfg)
    t_cpu = time.perf_counter() - t0
    curves = np.array(ev.deletion_curves, dtype=np.float64)
    dp = float(np.nanmax(np.abs(curves - np.array(ref_curves, dtype=np.float64))))
    same_nan = bool(np.array_equal(np.isnan(curves), np.isnan(np.array(ref_curves))))
    print("end to end deletion(x, y, 'wavelet', %d), %d clips, FtEx: device %.1f ms / call (mean of %d); "
          "CPU restatement on %d threads %.2f s; ratio %.0fx; max |dp| %.2e, NaN rows equal: %s"
          % (n_iter, n, 1e3 * t_dev, reps, a.threads, t_cpu, t_cpu / t_dev, dp, same_nan))
    assert len(scores) == n


if __name__ == "__main__":
    main()
