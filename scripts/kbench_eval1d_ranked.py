"""wam_waverec1_ranked + wam_peak_divide (wam_amd/csrc/evaluate1d.hip, k_dwt1_syn_ranked in dwt1_tile.hip)
beside the composition Eval1DWAM runs under its default layout, on the same tree, at the evaluation geometry
of config c3: clips of 80,000 samples, J = 5, n_iter = 64 (65 reconstructions per clip), haar and db6, for 1
and 8 clips. Three contenders compute the same peak-normalised [clips * 65, 80,000] reconstructions and silent
flags from the same coefficients and ranking (the identity slot map of mask_layout="coeffs"):

  composition  wam_rank_mask_coeffs -> wam_waverec -> wam_peak_normalize (in place): the parent's kernels
  route 0      wam_waverec1_ranked(route 0): the same expansion and synthesis, a max-only pass -> wam_peak_divide
  route 1      wam_waverec1_ranked(route 1): k_rank_table -> k_dwt1_syn_ranked, no masked coefficient stored,
               the maxima from the kernel's own reduction -> wam_peak_divide

Per geometry the contenders alternate over --rounds rounds; each round times --window seconds of calls per
contender with device events after a warm-up. Reported: the median (min, max) time per call over the rounds,
the bytes of the output alone (the floor every contender must write), the rate achieved on that floor and its
share of the 8 TB/s HBM peak, and the ratios of the medians. The outputs and flags are compared bit for bit.
One call per contender also runs with the library's per-launch timing on. The last lines state, per filter,
whether route 1's slowest round beat route 0's fastest at every clip count: the condition under which
wam_waverec1_ranked_route may answer 1 for that filter. --e2e adds Eval1DWAM.deletion(x, y, "wavelet", 64) of
8 haar clips under the default layout and under mask_layout="coeffs" (the same slices at this dyadic length).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8e12
NAMES = ("composition", "route 0", "route 1")


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


def end_to_end(dev, length, levels, n_iter, clips, rounds):
    import testmodels
    from wam_amd.evaluation import Eval1DWAM
    from wam_amd.plan import get_plan
    plan = get_plan(1, (length,), levels, "haar", "reflect", dev)
    rs = np.random.RandomState(3)
    x = torch.tensor(rs.standard_normal((clips, length)).astype(np.float32))
    y = [int(v) for v in rs.randint(0, 10, clips)]
    gw = (np.zeros((clips, 3, 32), np.float32), [rs.standard_normal((clips, s[0])).astype(np.float32)
                                                  for s in plan.band_shapes])
    evs = []
    for layout in ("reference", "coeffs"):
        ev = Eval1DWAM(testmodels.TinyAudio().to(dev), wavelet="haar", J=levels, n_mels=32, n_fft=256, sample_rate=16000,
                       n_samples=2, silent="zero", mask_layout=layout)
        ev.grad_wams = gw
        evs.append(ev)
    ms = [[], []]
    for r in range(rounds + 1):          # round 0 warms up
        for i, ev in enumerate(evs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.deletion(x, y, "wavelet", n_iter)
            torch.cuda.synchronize()
            if r:
                ms[i].append(1e3 * (time.perf_counter() - t0))
    same = np.array_equal(np.array(evs[0].deletion_curves), np.array(evs[1].deletion_curves))
    for i, layout in enumerate(("reference", "coeffs")):
        print("end to end: deletion(x, y, 'wavelet', %d) of %d haar clips, mask_layout=%-11s %8.1f ms (%.1f, %.1f), host "
              "clock around a synchronise" % (n_iter, clips, repr(layout), float(np.median(ms[i])), min(ms[i]), max(ms[i])))
    print("end to end: curves equal between the layouts: %s" % same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=80000)
    ap.add_argument("--n-iter", type=int, default=64)
    ap.add_argument("--clips", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--wavelets", nargs="+", default=["haar", "db6"])
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of timed calls per contender per round")
    ap.add_argument("--e2e", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_eval1d_ranked needs a HIP device"
    from wam_amd._lib import check, lib, ptr, stream_of
    from wam_amd.plan import get_plan, peak_divide, timing_drain, timing_enable

    dev = torch.device("cuda", 0)
    W, n_iter, J = a.length, a.n_iter, a.levels
    M = n_iter + 1
    print("wam_waverec1_ranked + wam_peak_divide: clips of %d samples, J = %d, n_iter = %d (%d reconstructions per clip); "
          "%d rounds, contenders alternating, %.1f s of calls per contender per round" % (W, J, n_iter, M, a.rounds, a.window))
    print("%-14s %-12s %28s  %6s  %10s  %9s  %s" % ("geometry", "contender", "median (min, max) per call", "reps",
                                                     "out bytes", "on floor", "share of 8 TB/s"))
    wins = {}
    for wavelet in a.wavelets:
        plan = get_plan(1, (W,), J, wavelet, "reflect", dev)
        K, n = plan.coeff_numel, plan.rec_shape[0]
        pos = torch.arange(K, dtype=torch.int32, device=dev)
        n_comp = int(K / n_iter)
        for clips in a.clips:
            g = torch.Generator().manual_seed(clips)
            x = torch.randn(clips, W, generator=g).to(dev)
            coeffs = plan.wavedec(x)
            rank = torch.stack([torch.randperm(K, device=dev) for _ in range(clips)]).to(torch.int32).contiguous()
            rows = clips * M
            outs = [torch.empty((rows, n), dtype=torch.float32, device=dev) for _ in range(3)]
            flags = [torch.full((rows,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
            masked = torch.empty(rows * K, dtype=torch.float32, device=dev)

            def composition():
                check(lib.wam_rank_mask_coeffs(plan.handle, clips, ptr(coeffs), ptr(rank), K, ptr(pos), n_iter, n_comp, 1,
                                               ptr(masked), stream_of(dev)))
                plan.waverec(masked, rows, out=outs[0].view(1, rows, n))
                check(lib.wam_peak_normalize(rows, n, ptr(outs[0]), ptr(outs[0]), ptr(flags[0]), 1, stream_of(dev)))

            def ranked(r):
                rec, mx = plan.waverec1_ranked(coeffs, clips, rank, pos, n_iter, n_comp, True, route=r, out=outs[1 + r])
                flags[1 + r] = peak_divide(rec, mx, zero_silent=True)[1]

            run = [composition, lambda: ranked(0), lambda: ranked(1)]
            for f in run:             # warm-up: code objects, the workspaces
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            same = all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:]) and \
                all(torch.equal(flags[0], f) for f in flags[1:])
            ms = [[], [], []]
            reps = [0, 0, 0]
            for _ in range(a.rounds):
                for i, f in enumerate(run):
                    t, reps[i] = timed(f, a.window)
                    ms[i].append(t)
            floor = 4.0 * rows * n
            med = [float(np.median(v)) for v in ms]
            geo = "%s %d clip%s" % (wavelet, clips, " " if clips == 1 else "s")
            for i in range(3):
                rate = floor / (med[i] * 1e-3)
                print("%-14s %-12s %9.1f us (%8.1f, %8.1f)  %6d  %7.1f MB  %6.0f GB/s  %5.1f %%"
                      % (geo, NAMES[i], 1e3 * med[i], 1e3 * min(ms[i]), 1e3 * max(ms[i]), reps[i], floor / 1e6,
                         rate / 1e9, 100 * rate / HBM_PEAK))
            win = max(ms[2]) < min(ms[1])
            wins.setdefault(wavelet, []).append(win)
            print("%-14s composition / route 0 = %.2fx, composition / route 1 = %.2fx, route 0 / route 1 = %.2fx; "
                  "outputs and flags bit-equal: %s; route 1's slowest round beats route 0's fastest: %s, the composition's "
                  "fastest: %s" % (geo, med[0] / med[1], med[0] / med[2], med[1] / med[2], same, win,
                                   max(ms[2]) < min(ms[0])))
            assert same, "the contenders differ"
            for i, f in enumerate(run):
                timing_enable(True)
                f()
                rec = timing_drain()
                timing_enable(False)
                tot = {}
                for n_, t, _ in rec:
                    tot[n_] = tot.get(n_, 0.0) + t
                print("    %s kernels: %s" % (NAMES[i], ", ".join("%s %.1f us" % (k, 1e3 * v) for k, v in tot.items())))
            del outs, coeffs, rank, masked, flags
            torch.cuda.empty_cache()
    for wavelet in a.wavelets:
        print("%s: route 1's slowest round beats route 0's fastest at every clip count: %s; route query "
              "(wam_waverec1_ranked_route) -> %d" % (wavelet, all(wins[wavelet]),
                                                     get_plan(1, (W,), J, wavelet, "reflect", dev).ranked1_route()))
    if a.e2e:
        end_to_end(dev, W, J, n_iter, 8, 3)


if __name__ == "__main__":
    main()
