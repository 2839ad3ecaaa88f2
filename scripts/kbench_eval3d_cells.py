"""The two routes of wam_waverec_cells (wam_amd/csrc/evaluate_cells.hip) on the same tree, at c5's geometry
-- haar J=2 on 128^3 volumes, 1 and 4 volumes x 128 masks on an 8^3 grid -- and at the reference's voxel
size, haar J=1 and J=2 on 16^3, 16 volumes x 128 masks on a 4^3 grid. Route 0 is the mask expansion
(k_cell_mask_coeffs3 over the plan's bands) into a workspace followed by wam_waverec; route 1 is
k_haar3_syn_cells. Then wam_gaussian_filter3d at 128^3, and one Eval3DWAM.mu_fidelity end to end per
geometry with cells_route 0 and 1 (TinyVoxel as the model, grad_wams handed over: the attribution is not
what is measured here).

Per geometry the routes alternate over --rounds rounds; each round times --window seconds of calls per
route with device events after a warm-up. Reported: the median (min, max) time per call over the rounds,
the bytes of the output alone (sets * masks * S^3 * 4: the floor either route must write), the rate
achieved on that floor and its share of the 8 TB/s HBM peak, and the ratio of the medians. The two outputs
are compared bit for bit. One call per route also runs with the library's per-launch timing on, to show
which kernels a route is made of. WAM_LIB_PATH=build/exp/<variant>.so measures a variant build (the
LDS-staged form of the fused kernel: WAM_CELLS_LDS 1 in kernels.hpp, scripts/build_variants.py).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8e12
# (S, J, sets, masks, grid)
GEOMETRIES = [(128, 2, 1, 128, 8), (128, 2, 4, 128, 8), (16, 1, 16, 128, 4), (16, 2, 16, 128, 4)]


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of timed calls per route per round")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end mu_fidelity runs")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_eval3d_cells needs a HIP device"
    import testmodels
    from wam_amd import _lib
    from wam_amd.evalcore import cell_map3, gaussian_weights
    from wam_amd.evaluation3d import Eval3DWAM, cube_pos_table
    from wam_amd.plan import gaussian_filter3d, get_plan, timing_drain, timing_enable

    dev = torch.device("cuda", 0)
    print("library: %s" % os.path.relpath(_lib.LIB_PATH))
    print("wam_waverec_cells: haar, float masks on a grid; %d rounds, routes alternating, %.1f s of calls per route "
          "per round" % (a.rounds, a.window))
    print("%-26s %-8s %28s  %6s  %10s  %9s  %s" % ("geometry", "route", "median (min, max) per call", "reps",
                                                    "out bytes", "on floor", "share of 8 TB/s"))
    faster = []
    for S, J, sets, M, g in GEOMETRIES:
        name = "%d^3 J=%d %2d x %d g=%d" % (S, J, sets, M, g)
        plan = get_plan(3, (S, S, S), J, "haar", "symmetric", dev)
        pos = torch.as_tensor(cube_pos_table(S, J, plan.band_shapes)).to(dev)
        slot = cell_map3(g, S, dev)[pos.long()].contiguous()
        x = testmodels.voxel_volumes(sets, S).to(dev)
        coeffs = plan.wavedec(x.view(sets, S, S, S))
        grid = torch.rand((sets, M, g ** 3), device=dev, generator=torch.Generator(dev).manual_seed(S + J + sets))
        outs = [torch.empty((sets * M, S, S, S), dtype=torch.float32, device=dev) for _ in range(2)]
        run = [lambda r=r: plan.waverec_cells(coeffs, sets, slot, grid, route=r, out=outs[r]) for r in (0, 1)]
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
            print("%-26s route %d  %9.1f us (%8.1f, %8.1f)  %6d  %7.1f MB  %6.0f GB/s  %5.1f %%"
                  % (name, r, 1e3 * med[r], 1e3 * min(ms[r]), 1e3 * max(ms[r]), reps[r], floor / 1e6, rate / 1e9,
                     100 * rate / HBM_PEAK))
        print("%-26s route 0 / route 1 = %.2fx; outputs bit-equal: %s" % (name, med[0] / med[1], same))
        assert same, "the two routes differ"
        faster.append(max(ms[1]) < min(ms[0]))
        for r in (0, 1):
            timing_enable(True)
            run[r]()
            rec = timing_drain()
            timing_enable(False)
            print("    route %d kernels: %s" % (r, ", ".join("%s %.1f us" % (n, 1e3 * t) for n, t, _ in rec)))
        del outs, coeffs, grid
        torch.cuda.empty_cache()
    print("route 1's slowest round beats route 0's fastest at every geometry: %s" % all(faster))
    print("route query (wam_waverec_cells_route): 128^3 J=2 -> %d, 16^3 J=1 -> %d" % (
        get_plan(3, (128,) * 3, 2, "haar", "symmetric", dev).cells_route,
        get_plan(3, (16,) * 3, 1, "haar", "symmetric", dev).cells_route))

    # ---- wam_gaussian_filter3d
    wts, radius = gaussian_weights(2.0)
    for items in (1, 4):
        vol = torch.randn((items, 128, 128, 128), dtype=torch.float64, device=dev)
        for _ in range(3):
            gaussian_filter3d(vol, wts, radius)
        ts = [timed(lambda: gaussian_filter3d(vol, wts, radius), a.window)[0] for _ in range(a.rounds)]
        nb = 3 * 16.0 * vol.numel()     # three passes, each reads and writes the volume
        print("wam_gaussian_filter3d %d x 128^3 float64, sigma 2 (radius %d): %8.1f us (%8.1f, %8.1f) per call, three "
              "passes, %.0f GB/s on their %.1f MB" % (items, radius, 1e3 * np.median(ts), 1e3 * min(ts), 1e3 * max(ts),
                                                       nb / (np.median(ts) * 1e-3) / 1e9, nb / 1e6))
        del vol

    # ---- mu_fidelity end to end
    if a.no_e2e:
        return
    model = testmodels.TinyVoxel().to(dev).eval()
    for S, J, n, M, g in [(128, 2, 1, 128, 8), (16, 1, 16, 128, 4), (16, 2, 16, 128, 4)]:
        x = testmodels.voxel_volumes(n, S)
        y = [i % 10 for i in range(n)]
        gw = np.random.RandomState(S).uniform(size=(n, S, S, S)).astype(np.float32)
        line = []
        for route in (0, 1):
            ev = Eval3DWAM(model, wavelet="haar", J=J)
            ev.grad_wams = gw
            ev.cells_route = route
            ts = []
            for _ in range(3):        # the first call warms the tables, the workspace and the model's kernels
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mu = ev.mu_fidelity(x, y, grid_size=g, sample_size=M)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            line.append("cells_route %d: %8.1f ms (first call %8.1f ms)" % (route, 1e3 * min(ts[1:]), 1e3 * ts[0]))
            del ev
            torch.cuda.empty_cache()
        print("mu_fidelity %d^3 J=%d, %2d volumes x %d masks, grid %d^3: %s; mu[0] = %.4f" % (S, J, n, M, g,
                                                                                              "; ".join(line), mu[0]))


if __name__ == "__main__":
    main()
