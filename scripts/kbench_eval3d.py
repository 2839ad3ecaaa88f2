"""The two routes of wam_waverec_ranked (wam_amd/csrc/evaluate_ranked.hip) on the same tree, at c5's evaluation
geometry -- haar J=2 on 128^3 volumes, n_iter = 64, so 65 reconstructions per volume, for 1 and 4 volumes
-- and at J=1. Route 0 is the mask expansion (k_rank_mask over the plan's bands) into a workspace followed
by wam_waverec, i.e. the kernels the tree had before the fused one; route 1 is k_haar3_syn_ranked.

Per geometry the routes alternate over --rounds rounds; each round times --window seconds of calls per
route with device events after a warm-up. Reported: the median (min, max) time per call over the rounds,
the bytes of the output alone (sets * (n_iter + 1) * S^3 * 4: the floor either route must write), the
rate achieved on that floor and its share of the 8 TB/s HBM peak, and the ratio of the medians. The two
outputs are compared bit for bit. One call per route also runs with the library's per-launch timing on,
to show which kernels a route is made of.
"""
import argparse
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--n-iter", type=int, default=64)
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 1])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of timed calls per route per round")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_eval3d needs a HIP device"
    import testmodels
    from wam_amd.evaluation3d import cube_pos_table
    from wam_amd.plan import get_plan, timing_drain, timing_enable

    dev = torch.device("cuda", 0)
    S, n_iter = a.size, a.n_iter
    M = n_iter + 1
    print("wam_waverec_ranked: haar on %d^3 volumes, n_iter = %d (%d reconstructions per volume); %d rounds, routes "
          "alternating, %.1f s of calls per route per round" % (S, n_iter, M, a.rounds, a.window))
    print("%-14s %-8s %28s  %6s  %10s  %9s  %s" % ("geometry", "route", "median (min, max) per call", "reps",
                                                    "out bytes", "on floor", "share of 8 TB/s"))
    for J in a.levels:
        plan = get_plan(3, (S, S, S), J, "haar", "symmetric", dev)
        K = plan.coeff_numel
        pos = torch.as_tensor(cube_pos_table(S, J, plan.band_shapes)).to(dev)
        for sets in a.sets:
            x = testmodels.voxel_volumes(sets, S).to(dev)
            coeffs = plan.wavedec(x.view(sets, S, S, S))
            rank = torch.stack([torch.randperm(K, device=dev) for _ in range(sets)]).to(torch.int32).contiguous()
            outs = [torch.empty((sets * M, S, S, S), dtype=torch.float32, device=dev) for _ in range(2)]
            run = [lambda r=r: plan.waverec_ranked(coeffs, sets, rank, pos, n_iter, int(K / n_iter), True, route=r,
                                                   out=outs[r]) for r in (0, 1)]
            for r in (0, 1):          # warm-up: code objects, the workspace
                for _ in range(3):
                    run[r]()
            torch.cuda.synchronize()
            same = torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
            ms = [[], []]
            reps = [0, 0]
            for _ in range(a.rounds):
                for r in (0, 1):
                    t, reps[r] = timed(run[r], a.window)
                    ms[r].append(t)
            floor = 4.0 * sets * M * S ** 3
            med = [float(np.median(v)) for v in ms]
            for r in (0, 1):
                rate = floor / (med[r] * 1e-3)
                print("J=%d %d set%s   route %d  %9.1f us (%8.1f, %8.1f)  %6d  %7.1f MB  %6.0f GB/s  %5.1f %%"
                      % (J, sets, " " if sets == 1 else "s", r, 1e3 * med[r], 1e3 * min(ms[r]), 1e3 * max(ms[r]), reps[r],
                         floor / 1e6, rate / 1e9, 100 * rate / HBM_PEAK))
            print("J=%d %d set%s   route 0 / route 1 = %.2fx; outputs bit-equal: %s" % (J, sets, " " if sets == 1 else "s",
                                                                                       med[0] / med[1], same))
            assert same, "the two routes differ"
            for r in (0, 1):
                timing_enable(True)
                run[r]()
                rec = timing_drain()
                timing_enable(False)
                print("    route %d kernels: %s" % (r, ", ".join("%s %.1f us" % (n, 1e3 * t) for n, t, _ in rec)))
            del outs, coeffs, rank
            torch.cuda.empty_cache()
    print("route query (wam_waverec_ranked_route): J=2 -> %d, J=1 -> %d" % tuple(
        get_plan(3, (S, S, S), J, "haar", "symmetric", dev).ranked_route for J in (2, 1)))


if __name__ == "__main__":
    main()
