"""The WAMAnalyzer2D kernels (wam_amd/csrc/analyze2d.hip) at the analyzer's working geometry -- 16 images
of 224 x 224, haar J=3, 32 quantiles, so 512 model inputs -- and one ``isolate_necessary_components``
call against the per-image CPU loop of the numpy restatement (tests/analyzer_ref.py on oracle/dwt.py).

Three measurements:
  1. per kernel, from the library's own launch records (WamTimer: device events around every launch, the
     algorithmic bytes from the shapes -- every input read once, every output written once): the median
     time over --reps calls after a warm-up, achieved bytes/s and its share of the 8 TB/s HBM peak. Both
     kernels are bandwidth-bound, so the share of peak is bytes / 8 TB/s over the kernel time;
  2. the same masked reconstructions made two ways, interleaved A B A B in one process: the batched path
     (wam_threshold_mask_coeffs on all images + one wam_waverec) and the existing per-image composition
     (float masks stored in memory, wam_coeff_masks and wam_waverec once per image), device events around
     each whole path; the outputs are compared bit for bit first;
  3. end to end: one isolate_necessary_components call on the device (mean of --calls after a warm-up,
     host clock around a device synchronise) against the CPU loop on --cpu-images images, scaled to all.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8e12


def kernel_rows(records, names):
    for name in names:
        ms = np.array([r[1] for r in records if r[0] == name])
        nb = [r[2] for r in records if r[0] == name]
        if not len(ms):
            print("%-22s no launch recorded" % name)
            continue
        med = float(np.median(ms))
        rate = nb[0] / (med * 1e-3)
        print("%-22s median %8.1f us (min %.1f, max %.1f) x %4d  %8.1f MB  %7.0f GB/s  %5.1f %% of 8 TB/s"
              % (name, 1e3 * med, 1e3 * ms.min(), 1e3 * ms.max(), len(ms), nb[0] / 1e6, rate / 1e9,
                 100 * rate / HBM_PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--quantiles", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=20, help="A B rounds of the interleaved comparison")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cpu-images", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the CPU restatement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_analyzer needs a HIP device"
    import testmodels
    from tests import analyzer_ref as R
    from tests.golden.analyzer_cases import make_image, make_map
    from wam_amd import WAMAnalyzer2D
    from wam_amd._lib import c_f32, check, lib, ptr, stream_of
    from wam_amd.analysis import masked_reconstructions, quantile_thresholds
    from wam_amd.evaluation import IMAGENET_MEAN, IMAGENET_STD, array_layout
    from wam_amd.plan import get_plan, timing_drain, timing_enable

    dev = torch.device("cuda", 0)
    N, S, J, Q = a.images, a.size, a.levels, a.quantiles
    qs = np.linspace(1.0, 0.0, Q).tolist()
    plan = get_plan(2, (S, S), J, "haar", "symmetric", dev)
    pos, shape = array_layout(plan, dev)
    K = plan.coeff_numel
    planes = torch.stack([torch.as_tensor(np.moveaxis(make_image(S, 1000 + n), 2, 0)) for n in range(N)]).to(dev)
    wams = np.stack([make_map(S, 2000 + n) for n in range(N)])
    maps = torch.as_tensor(wams).to(dev).reshape(N, -1).contiguous()
    thr = quantile_thresholds(maps, qs)
    coeffs = plan.wavedec(planes)
    st = stream_of(dev)
    print("geometry: %d images x 3 x %d^2, haar J=%d, %d quantiles -> %d model inputs, %d coefficients per plane"
          % (N, S, J, Q, N * Q, K))

    # ---- 1. the two kernels, from the launch records
    masked = torch.empty(N * Q * 3 * K, dtype=torch.float32, device=dev)

    def threshold():
        check(lib.wam_threshold_mask_coeffs(plan.handle, N, 3, ptr(coeffs), ptr(pos), S, ptr(maps), Q, ptr(thr), Q, 0,
                                            None, 0, ptr(masked), st))

    threshold()
    rec = plan.waverec(masked, N * Q * 3)[0].view(N * Q, 3, S * S)
    u8 = torch.empty((N * Q, 3, S * S), dtype=torch.uint8, device=dev)
    out = torch.empty((N * Q, 3, S * S), dtype=torch.float32, device=dev)
    mean, std = (c_f32 * 3)(*IMAGENET_MEAN), (c_f32 * 3)(*IMAGENET_STD)

    def quantize():
        check(lib.wam_quantize_normalize_ex(N * Q, 3, S * S, ptr(rec), 1, mean, std, ptr(u8), ptr(out), st))

    for _ in range(5):
        threshold(), quantize()
    torch.cuda.synchronize()
    timing_enable(True)
    timing_drain()
    for _ in range(a.reps):
        threshold(), quantize()
    torch.cuda.synchronize()
    records = timing_drain()
    timing_enable(False)
    kernel_rows(records, ["k_threshold_mask", "k_quantize_analyzer"])

    # ---- 2. batched path vs the per-image composition, interleaved
    def batched():
        return masked_reconstructions(plan, pos, S, planes, maps, thr)

    def composition(keep=None):
        for n in range(N):
            masks = (maps[n][None, :] >= thr[n][:, None]).to(torch.float32).contiguous()   # stored float masks
            c = plan.wavedec(planes[n])
            m = torch.empty(Q * 3 * K, dtype=torch.float32, device=dev)
            check(lib.wam_coeff_masks(plan.handle, 3, ptr(c), ptr(pos), Q, S * S, ptr(masks), ptr(m), st))
            r = plan.waverec(m, Q * 3)[0]
            if keep is not None:
                keep.append(r.view(Q, 3, S, S))
        return keep

    same = torch.equal(batched(), torch.stack(composition([])))
    print("batched and per-image reconstructions bit-equal: %s" % same)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tb, tc = [], []
    for _ in range(3):
        batched(), composition()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        ev[0].record()
        batched()
        ev[1].record()
        composition()
        ev[2].record()
        torch.cuda.synchronize()
        tb.append(ev[0].elapsed_time(ev[1]))
        tc.append(ev[1].elapsed_time(ev[2]))
    tb, tc = np.array(tb), np.array(tc)
    print("masked reconstructions of %d images x %d quantiles, %d interleaved rounds: batched median %.3f ms "
          "(min %.3f, max %.3f); per-image composition median %.3f ms (min %.3f, max %.3f); ratio %.2fx"
          % (N, Q, a.rounds, np.median(tb), tb.min(), tb.max(), np.median(tc), tc.min(), tc.max(),
             np.median(tc) / np.median(tb)))

    # ---- 3. end to end
    model = testmodels.TinySmooth2D()
    x = planes.cpu()
    y = [8] * N
    an = WAMAnalyzer2D(model.to(dev), wavelet="haar", J=J)
    an.grad_wams = wams
    an.isolate_necessary_components(x, y, qs, mode="insertion")   # warm-up: plans, tables, MIOpen's algorithm search
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        outs = an.isolate_necessary_components(x, y, qs, mode="insertion")
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / a.calls
    torch.set_num_threads(a.threads)
    nc = max(1, min(a.cpu_images, N))
    t0 = time.perf_counter()
    ref_outs, _ = R.isolate_necessary_components(testmodels.TinySmooth2D(), x[:nc], y[:nc], wams[:nc], qs, "insertion", J)
    t_cpu = (time.perf_counter() - t0) * N / nc
    dp = max((float(np.abs(o[3][0] - r[3][0]).max()) for o, r in zip(outs, ref_outs)
              if r[1] is not None and o[1] is not None),
             default=float("nan"))
    print("end to end isolate_necessary_components, %d images x %d quantiles, TinySmooth2D: device %.1f ms / call "
          "(mean of %d); CPU restatement %.2f s (measured on %d images on %d threads, scaled to %d); ratio %.0fx; "
          "max |dp| on the compared images %.2e"
          % (N, Q, 1e3 * t_dev, a.calls, t_cpu, nc, a.threads, N, t_cpu / t_dev, dp))


if __name__ == "__main__":
    main()
