"""wam_waverec2_ranked (wam_amd/csrc/evaluate_ranked.hip) beside the composition Eval2DWAM ran before it, on the
same tree, at the evaluation geometry of the headline configurations: 224 x 224 images of 3 channels,
n_iter = 64 (65 reconstructions per image), haar J=3 and db4 J=3, for 1 and 4 images. Three contenders
compute the same [images, 65, 3, 224, 224] reconstructions from the same coefficients, ranking and mosaic
slot map (frames.wam_cell_source, the held slot appended):

  composition  per image wam_rank_masks -> wam_coeff_masks -> wam_waverec: the float masks are stored
  route 0      k_rank_mask (the shared mask expansion, timer label "k_rank_mask2") into the workspace -> wam_waverec
  route 1      k_rank_table -> k_plane_syn_ranked: no masked coefficient is stored

Per geometry the contenders alternate over --rounds rounds; each round times --window seconds of calls per
contender with device events after a warm-up. Reported: the median (min, max) time per call over the
rounds, the bytes of the output alone (the floor every contender must write), the rate achieved on that
floor and its share of the 8 TB/s HBM peak, and the ratios of the medians. The three outputs are compared
bit for bit. One call per contender also runs with the library's per-launch timing on. The last lines
state whether route 1's slowest round beat the composition's fastest at every geometry: the condition
under which wam_waverec2_ranked_route may answer 1.
"""
import argparse
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--n-iter", type=int, default=64)
    ap.add_argument("--images", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--wavelets", nargs="+", default=["haar", "db4"])
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of timed calls per contender per round")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_eval2d needs a HIP device"
    from wam_amd._lib import check, lib, ptr, stream_of
    from wam_amd.frames import wam_cell_source
    from wam_amd.plan import get_plan, timing_drain, timing_enable

    dev = torch.device("cuda", 0)
    S, n_iter, C, J = a.size, a.n_iter, 3, a.levels
    M = n_iter + 1
    print("wam_waverec2_ranked: %d x %d images of %d channels, J = %d, n_iter = %d (%d reconstructions per image); "
          "%d rounds, contenders alternating, %.1f s of calls per contender per round"
          % (S, S, C, J, n_iter, M, a.rounds, a.window))
    print("%-16s %-12s %28s  %6s  %10s  %9s  %s" % ("geometry", "contender", "median (min, max) per call", "reps",
                                                     "out bytes", "on floor", "share of 8 TB/s"))
    wins = []
    for wavelet in a.wavelets:
        plan = get_plan(2, (S, S), J, wavelet, "symmetric", dev)
        K = plan.coeff_numel
        src, (hc, wc) = wam_cell_source(plan, "native", "smooth")
        cells = hc * wc
        shown = np.flatnonzero(src.reshape(-1) >= 0)
        pos_h = np.full(K, cells, dtype=np.int32)
        pos_h[src.reshape(-1)[shown]] = shown
        pos = torch.as_tensor(pos_h).to(dev)
        n_comp = int(cells / n_iter)
        rh, rw = plan.rec_shape
        for images in a.images:
            g = torch.Generator().manual_seed(images)
            x = torch.rand(images, C, S, S, generator=g).to(dev)
            coeffs = plan.wavedec(x)
            per_image = [plan.wavedec(x[n]).clone() for n in range(images)]
            rank = torch.stack([torch.randperm(cells, device=dev) for _ in range(images)]).to(torch.int32)
            rank = torch.cat([rank, torch.full((images, 1), -1, dtype=torch.int32, device=dev)], 1).contiguous()
            outs = [torch.empty((images, M, C, rh, rw), dtype=torch.float32, device=dev) for _ in range(3)]
            masks = torch.empty((M, cells + 1), dtype=torch.float32, device=dev)
            masked = torch.empty(M * C * K, dtype=torch.float32, device=dev)

            def composition():
                for n in range(images):
                    check(lib.wam_rank_masks(n_iter, n_comp, cells + 1, ptr(rank[n]), 0, ptr(masks), stream_of(dev)))
                    check(lib.wam_coeff_masks(plan.handle, C, ptr(per_image[n]), ptr(pos), M, cells + 1, ptr(masks),
                                              ptr(masked), stream_of(dev)))
                    plan.waverec(masked, M * C, out=outs[0][n].view(1, M * C, rh, rw))

            run = [composition] + [lambda r=r: plan.waverec2_ranked(coeffs, images, C, rank, pos, n_iter, n_comp, False,
                                                                    route=r, out=outs[1 + r]) for r in (0, 1)]
            for f in run:             # warm-up: code objects, the workspaces
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            same = all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
            ms = [[], [], []]
            reps = [0, 0, 0]
            for _ in range(a.rounds):
                for i, f in enumerate(run):
                    t, reps[i] = timed(f, a.window)
                    ms[i].append(t)
            floor = 4.0 * images * M * C * rh * rw
            med = [float(np.median(v)) for v in ms]
            geo = "%s %d image%s" % (wavelet, images, " " if images == 1 else "s")
            for i in range(3):
                rate = floor / (med[i] * 1e-3)
                print("%-16s %-12s %9.1f us (%8.1f, %8.1f)  %6d  %7.1f MB  %6.0f GB/s  %5.1f %%"
                      % (geo, NAMES[i], 1e3 * med[i], 1e3 * min(ms[i]), 1e3 * max(ms[i]), reps[i], floor / 1e6,
                         rate / 1e9, 100 * rate / HBM_PEAK))
            win = max(ms[2]) < min(ms[0])
            wins.append(win)
            print("%-16s composition / route 0 = %.2fx, composition / route 1 = %.2fx, route 0 / route 1 = %.2fx; "
                  "outputs bit-equal: %s; route 1's slowest round beats the composition's fastest: %s"
                  % (geo, med[0] / med[1], med[0] / med[2], med[1] / med[2], same, win))
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
            del outs, coeffs, rank, masks, masked, per_image
            torch.cuda.empty_cache()
    print("route 1 beats the composition in every round at every geometry: %s" % all(wins))
    print("route query (wam_waverec2_ranked_route): %s" % ", ".join(
        "%s -> %d" % (w, get_plan(2, (S, S), J, w, "symmetric", dev).ranked2_route()) for w in a.wavelets))


if __name__ == "__main__":
    main()
