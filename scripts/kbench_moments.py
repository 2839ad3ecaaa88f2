"""The second-moment epilogue kernels (wam_amd/csrc/epilogue.hip) at two geometries:

  c2: 64 images x 25 samples, db4 J=3 at 224^2, native frame, normalised, coefficient order
  c5: 16 volumes x 25 samples, haar J=2 at 128^3

For each, three things are timed on the same buffers:
  (a) the moment kernel (wam_frame_moments_coef / wam_cube_moments): S and Q from one pass over the maps;
  (b) the existing single-sum kernel (wam_frame_accumulate_coef / wam_cube_accumulate, weights of 1), for scale;
  (c) the composition one would build from the parts the library had before: an elementwise square of
      the maps (and of the band maxima) into a second buffer, then two single-sum calls.
The three alternate over --rounds rounds; each round times --window seconds of calls per variant with
device events after a warm-up. Reported: the median (min, max) per call, the algorithmic bytes (the
library's own count, from its per-launch timing records; for (c) the square's 8 bytes per map value on
top of two sums) and the rate on them as a share of the 8 TB/s HBM peak, then (c) / (a).

--call also times whole calls of WaveletAttribution2D with method 'smooth' and 'vargrad' at c2's shape
(resnet50, Philox noise, native frame); informational.
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
    """ms per call over enough repetitions to fill `window` seconds, with device events."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    iters = max(5, int(window * 1e3 / max(s.elapsed_time(e), 1e-3)))
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, iters


def lib_bytes(fn):
    """algorithmic bytes of the library launches of one (warm) call"""
    from wam_amd.plan import timing_drain, timing_enable
    fn()
    timing_enable(True)
    fn()
    rec = timing_drain()
    timing_enable(False)
    return sum(b for _, _, b in rec), ", ".join("%s %.1f us" % (n, 1e3 * t) for n, t, _ in rec)


def report(geom, variants, rounds, window):
    """variants: [(label, fn, bytes)]"""
    for _, fn, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in variants]
    reps = [0] * len(variants)
    for _ in range(rounds):
        for i, (_, fn, _) in enumerate(variants):
            t, reps[i] = timed(fn, window)
            ms[i].append(t)
    med = [float(np.median(v)) for v in ms]
    for i, (label, _, nbytes) in enumerate(variants):
        rate = nbytes / (med[i] * 1e-3)
        print("%-4s %-34s %9.1f us (%8.1f, %8.1f)  %6d  %8.1f MB  %6.0f GB/s  %5.1f %%"
              % (geom, label, 1e3 * med[i], 1e3 * min(ms[i]), 1e3 * max(ms[i]), reps[i], nbytes / 1e6, rate / 1e9,
                 100 * rate / HBM_PEAK))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of timed calls per variant per round")
    ap.add_argument("--call", action="store_true", help="also time whole 'smooth' / 'vargrad' calls at c2's shape")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_moments needs a HIP device"
    from wam_amd import frames
    from wam_amd import plan as P

    dev = torch.device("cuda", 0)
    print("second-moment epilogue: %d rounds, variants alternating, %.1f s of calls per variant per round" % (
        a.rounds, a.window))
    print("%-4s %-34s %31s  %6s  %11s  %11s  %s" % ("geom", "variant", "median (min, max) per call", "reps", "alg. bytes",
                                                     "rate", "share of 8 TB/s"))
    # ---- c2
    n, g = 64, 25
    p = P.get_plan(2, (224, 224), 3, "db4", "reflect", dev)
    K, nb = p.coeff_numel, p.nbands
    gmap, (rh, rw) = frames.smooth_frame(p, n, "native", dev)
    assert P._inverse_map(gmap, K) is not None  # coefficient order
    maps = torch.rand(g * n * K, device=dev) + 0.05
    bmax = torch.rand(g, nb, device=dev) + 1.0
    maps2, bmax2 = torch.empty_like(maps), torch.empty_like(bmax)
    S, Q = (torch.zeros(n * rh * rw, dtype=torch.float64, device=dev) for _ in range(2))

    def c2_moments():
        P.frame_moments(g, n, gmap, maps, K, bmax, nb, True, S, Q)

    def c2_sum():
        P.frame_accumulate(g, n, gmap, maps, K, bmax, nb, True, S)

    def c2_composed():
        torch.mul(maps, maps, out=maps2)
        torch.mul(bmax, bmax, out=bmax2)
        P.frame_accumulate(g, n, gmap, maps, K, bmax, nb, True, S)
        P.frame_accumulate(g, n, gmap, maps2, K, bmax2, nb, True, Q)

    b_m, k_m = lib_bytes(c2_moments)
    b_s, k_s = lib_bytes(c2_sum)
    med = report("c2", [("(a) wam_frame_moments_coef", c2_moments, b_m), ("(b) wam_frame_accumulate_coef", c2_sum, b_s),
                        ("(c) square + 2 x accumulate_coef", c2_composed, 2 * b_s + 8.0 * maps.numel())],
                 a.rounds, a.window)
    print("c2   (c) / (a) = %.2fx; kernels: %s | %s" % (med[2] / med[0], k_m, k_s))
    del maps, maps2, S, Q
    torch.cuda.empty_cache()
    # ---- c5
    n, g, size = 16, 25, 128
    p3 = P.get_plan(3, (size,) * 3, 2, "haar", "symmetric", dev)
    K3 = p3.coeff_numel
    src = frames.cube_map(p3, size, dev)
    maps = torch.rand(g * n * K3, device=dev)
    maps2 = torch.empty_like(maps)
    S, Q = (torch.zeros(n * size ** 3, dtype=torch.float64, device=dev) for _ in range(2))
    A, B = (torch.zeros(n * size ** 3, dtype=torch.float32, device=dev) for _ in range(2))
    ones = torch.ones(g, device=dev)

    def c5_moments():
        P.cube_moments(g, n, src, maps, K3, S, Q)

    def c5_sum():
        P.cube_accumulate(g, 0, n, src, maps, K3, 1, 1.0, A, weights=ones)

    def c5_composed():
        torch.mul(maps, maps, out=maps2)
        P.cube_accumulate(g, 0, n, src, maps, K3, 1, 1.0, A, weights=ones)
        P.cube_accumulate(g, 0, n, src, maps2, K3, 1, 1.0, B, weights=ones)

    b_m, k_m = lib_bytes(c5_moments)
    b_s, k_s = lib_bytes(c5_sum)
    med = report("c5", [("(a) wam_cube_moments", c5_moments, b_m), ("(b) wam_cube_accumulate (w = 1)", c5_sum, b_s),
                        ("(c) square + 2 x cube_accumulate", c5_composed, 2 * b_s + 8.0 * maps.numel())],
                 a.rounds, a.window)
    print("c5   (c) / (a) = %.2fx; kernels: %s | %s" % (med[2] / med[0], k_m, k_s))
    print("note: (b) and (c) of c5 keep float32 accumulators (what wam_cube_accumulate has); (a) keeps float64 ones")
    del maps, maps2, S, Q, A, B
    torch.cuda.empty_cache()
    if not a.call:
        return
    # ---- whole calls at c2's shape (informational)
    import testmodels
    from wam_amd import WaveletAttribution2D
    x = torch.rand(64, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    y = [int(v) for v in np.random.RandomState(0).randint(0, 1000, 64)]
    model = testmodels.resnet50().cuda().eval()
    ex = {m: WaveletAttribution2D(model, wavelet="db4", J=3, method=m, n_samples=25, noise="philox", frame="native")
          for m in ("smooth", "vargrad")}
    wall = {m: [] for m in ex}
    for r in range(4):
        for m in ex:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ex[m](x, y)
            torch.cuda.synchronize()
            if r:  # round 0 warms up
                wall[m].append(time.perf_counter() - t0)
    for m in ex:
        print("call c2 (resnet50, 64 x 25, db4 J=3, philox, native) method=%-8s %8.1f ms (%8.1f, %8.1f) over 3 calls"
              % (m, 1e3 * np.median(wall[m]), 1e3 * min(wall[m]), 1e3 * max(wall[m])))
    print("call c2 vargrad / smooth = %.3fx" % (np.median(wall["vargrad"]) / np.median(wall["smooth"])))


if __name__ == "__main__":
    main()
