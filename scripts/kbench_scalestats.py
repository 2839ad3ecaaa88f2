"""The scale-statistics kernels (wam_amd/csrc/scalestats.hip) at the sizes wam_amd.utils meets, beside the
reference's host loop.

Three measurements:
  1. wam_level_stats on 64 x 224^2 at J = 3 (one c2 call's maps) and 16 x 512^2 at J = 5, both `size` values:
     the ranking form (mean_var only, no variance map stored) and the full form (abs_sums + var_map +
     mean_var), interleaved rounds with device events around each whole call; then each kernel's own
     time from the library's launch records with the achieved bytes/s on its algorithmic bytes (the
     diagonal blocks read once, the outputs and partial sums written once).
  2. rank_images end to end (wall clock, mean of --calls calls, result on the host) from maps already on
     the device and from a numpy array (one upload), against the reference's loop on the host:
     scipy.ndimage.zoom + np.var per image (tests/scalestats_ref.py's restatement of it where scipy is
     missing) over ALL images, median of --host-repeats passes, once on one thread as the reference runs
     it and once spread over --threads worker processes (the loop has no parallelism of its own; the
     maps are pickled to the workers, which is part of that figure).
  3. mean_pairwise_iou for 6 maps x 10 percentages at 224^2: the whole call (device sort for the order
     statistics, one wam_mask_iou launch, counts to the host; wall clock, mean of --calls calls),
     k_mask_iou's own time, and the notebook's host loop (argsort per map and percentage, boolean
     reductions per pair; one thread, median of --host-repeats passes).

Every host figure is taken before the process touches the GPU: the worker processes are started and
joined first.
"""
import argparse
import multiprocessing
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from kbench_baselines import interleaved, kernel_rows  # noqa: E402

PERCENTAGES = (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5)


GEOMETRIES = ((64, 224, 3), (16, 512, 5))
SIZES = ("maximal", "minimal")


def host_mean_variance(job):
    """The reference's get_mean_pixelwise_variance of one map on the host (a pool worker's job)."""
    wam, J, size = job
    from tests import scalestats_ref as R
    try:
        from scipy.ndimage import zoom
    except ImportError:
        return R.mean_variance(wam, J, size)
    levels = R.diagonal(wam, J)[:J]
    T = R.target_side(wam.shape[0], J, size)
    stack = np.stack([zoom(b, T / b.shape[0], order=1)[:T, :T] for b in levels], axis=0)
    return float(np.mean(np.var(stack, axis=0)))


def median_time(f, repeats):
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def host_measurements(data, iou_maps, threads, repeats):
    """{(N, S, J, size): (one-thread s, pool s, values)} and (iou s, iou values), before any GPU work."""
    from tests import scalestats_ref as R
    res = {}
    with multiprocessing.get_context("spawn").Pool(threads) as pool:
        pool.map(host_mean_variance, [(np.zeros((8, 8)), 1, "maximal")] * (4 * threads))   # workers up, imports done
        for (N, S, J), host in data.items():
            for size in SIZES:
                jobs = [(m, J, size) for m in host]
                t1, vals = median_time(lambda: [host_mean_variance(j) for j in jobs], repeats)
                tp, vals_p = median_time(lambda: pool.map(host_mean_variance, jobs, 1), repeats)
                assert vals == vals_p
                res[N, S, J, size] = (t1, tp, vals)
    t_iou, counts = median_time(lambda: R.pair_counts(iou_maps, PERCENTAGES), repeats)
    return res, (t_iou, R.mean_iou(*counts))


def wall(f, calls):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16, help="worker processes of the parallel host loop")
    ap.add_argument("--host-repeats", type=int, default=5)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    data = {g: rs.standard_normal((g[0], g[1], g[1])) for g in GEOMETRIES}
    M, S_IOU = 6, 224
    iou_maps = rs.standard_normal((M, S_IOU, S_IOU))
    host_res, (t_iou_host, iou_ref) = host_measurements(data, iou_maps, a.threads, a.host_repeats)

    assert torch.cuda.is_available(), "kbench_scalestats needs a HIP device"
    from tests import scalestats_ref as R
    from wam_amd import utils as U
    from wam_amd.plan import timing_drain, timing_enable
    try:
        import scipy.ndimage  # noqa: F401
        loop = "scipy.ndimage.zoom + np.var"
    except ImportError:
        loop = "numpy restatement of scipy's zoom + np.var"
    print("host loop: %s over all images, median of %d passes: on one thread, and over %d worker processes"
          % (loop, a.host_repeats, a.threads))

    for (N, S, J), host in data.items():
        dev = torch.as_tensor(host).cuda()
        sides = R.detail_sides(S, J)
        detail = 8.0 * N * sum(n * n for n in sides)
        for size in SIZES:
            T = R.target_side(S, J, size)
            what = "%d x %d^2, J = %d, %s (T = %d)" % (N, S, J, size, T)
            paths = {"rank": lambda: U._level_stats(dev, J, size, want_mean=True),
                     "full": lambda: U._level_stats(dev, J, size, want_abs=True, want_map=True, want_mean=True)}
            res = interleaved(paths, a.rounds)
            for k, (med, lo, hi) in res.items():
                print("wam_level_stats %s, %d interleaved rounds: %-4s median %.3f ms (min %.3f, max %.3f)"
                      % (what, a.rounds, k, med, lo, hi))
            timing_enable(True)
            timing_drain()
            for _ in range(a.rounds):
                paths["full"]()
            torch.cuda.synchronize()
            kernel_rows(timing_drain(), ["k_level_abs", "k_level_var", "k_level_finish"])
            timing_enable(False)
            print("  algorithmic bytes of the full form: detail blocks %.2f MB read by each of k_level_abs and "
                  "k_level_var, var_map %.2f MB written" % (detail / 1e6, 8.0 * N * T * T / 1e6))
            t_dev = wall(lambda: U.rank_images(dev, J, size=size), a.calls)
            t_up = wall(lambda: U.rank_images(host, J, size=size), a.calls)
            t_one, t_pool, ref = host_res[N, S, J, size]
            got = {r["image_index"]: r["mean_pixelwise_variance"] for r in U.rank_images(dev, J, size=size)}
            err = max(abs(got[i] - ref[i]) / abs(ref[i]) for i in range(N)) / R.U
            print("rank_images %s: device maps %.3f ms / call, numpy maps (%.1f MB uploaded) %.3f ms / call (wall, mean "
                  "of %d); host loop over %d images, median of %d: one thread %.1f ms, %d processes %.1f ms; one thread / "
                  "device %.0fx (%.0fx from numpy), %d processes / device %.0fx (%.0fx from numpy); max relative "
                  "|d mean_var| %.2f u"
                  % (what, 1e3 * t_dev, 8.0 * N * S * S / 1e6, 1e3 * t_up, a.calls, N, a.host_repeats, 1e3 * t_one,
                     a.threads, 1e3 * t_pool, t_one / t_dev, t_one / t_up, a.threads, t_pool / t_dev, t_pool / t_up,
                     err))

    S, maps = S_IOU, iou_maps
    dev = torch.as_tensor(maps).cuda()
    t_dev = wall(lambda: U.mean_pairwise_iou(dev, PERCENTAGES), a.calls)
    t_up = wall(lambda: U.mean_pairwise_iou(maps, PERCENTAGES), a.calls)
    timing_enable(True)
    timing_drain()
    for _ in range(a.rounds):
        U.mean_pairwise_iou(dev, PERCENTAGES)
    torch.cuda.synchronize()
    kernel_rows(timing_drain(), ["k_mask_iou"])
    timing_enable(False)
    t_cpu, ref = t_iou_host, iou_ref
    same = np.array_equal(U.mean_pairwise_iou(dev, PERCENTAGES), ref)
    print("mean_pairwise_iou, %d maps x %d percentages at %d^2 (%d pairs): device maps %.3f ms / call, numpy maps %.3f "
          "ms / call (wall, mean of %d: device sort + k_mask_iou + counts to the host); the notebook's host loop, one thread, "
          "median of %d, %.1f ms; host / device %.0fx; equal floats: %s; the maps are %.1f MB"
          % (M, len(PERCENTAGES), S, M * (M - 1) // 2, 1e3 * t_dev, 1e3 * t_up, a.calls, a.host_repeats, 1e3 * t_cpu,
             t_cpu / t_dev, same, 8.0 * M * S * S / 1e6))
    assert same


if __name__ == "__main__":
    main()
