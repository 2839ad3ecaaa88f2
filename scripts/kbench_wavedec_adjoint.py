"""The wavedec adjoint kernels (wam_amd/csrc/dwt_adjoint.hip; the backward pass of wam_wavedec) at four
geometries, written to profiles/wavedec_adjoint_kbench.txt.

Two measurements per 2D geometry (192 planes of 224^2, db4 J=3; 384 planes of 512^2, sym8 J=5; reflect):
  1. per kernel and level, from the library's own launch records (WamTimer: device events around every
     launch, the algorithmic bytes from the shapes -- every input read once, every output written once):
     the median time over --reps calls after a warm-up, achieved bytes/s and its share of the 8 TB/s HBM
     peak, for the fold route (k_dwt2_syn + k_dwt2_adjoint_border per level) and for the axis route
     (k_analysis_adjoint_axis, three launches per level);
  2. whole calls, interleaved A B C A B C in one process with device events around each: the fold route,
     the axis route (the same plan built with generic=True) and wam_waverec on the fold plan -- the
     yardstick, since it moves the same algorithmic bytes. The two routes' outputs are compared first.
On the axis route alone (1D and 3D plans have no other): 256 signals of 80,000 samples, db6 J=5, and 16
volumes of 128^3, haar J=2, with wam_waverec of the same plan beside them.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8e12
LINES = []


def emit(s):
    print(s, flush=True)
    LINES.append(s)


def kernel_rows(records, label, reps):
    """One row per launch of a call, in launch order (every call issues the same sequence)."""
    per_call = len(records) // reps
    total = 0.0
    for i in range(per_call):
        name, nb = records[i][0], records[i][2]
        ms = np.array([r[1] for r in records[i::per_call]])
        assert all(r[0] == name for r in records[i::per_call])
        med = float(np.median(ms))
        total += med
        rate = nb / (med * 1e-3)
        emit("  %-6s %-24s median %8.1f us (min %.1f, max %.1f) x %4d  %8.1f MB  %7.0f GB/s  %5.1f %% of 8 TB/s"
             % (label, name, 1e3 * med, 1e3 * ms.min(), 1e3 * ms.max(), len(ms), nb / 1e6, rate / 1e9,
                100 * rate / HBM_PEAK))
    emit("  %-6s sum of the kernel medians %.1f us" % (label, 1e3 * total))


def records_of(P, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    P.timing_enable(True)
    P.timing_drain()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rec = P.timing_drain()
    P.timing_enable(False)
    return rec


def interleaved(fns, rounds):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        ev[0].record()
        for i, f in enumerate(fns):
            f()
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i in range(len(fns)):
            t[i].append(ev[i].elapsed_time(ev[i + 1]))
    return [np.array(v) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=30, help="rounds of the interleaved comparison")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "wavedec_adjoint_kbench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_wavedec_adjoint needs a HIP device"
    from wam_amd import plan as P

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    fmt = lambda v: "median %.1f us (min %.1f, max %.1f)" % (1e3 * np.median(v), 1e3 * v.min(), 1e3 * v.max())

    for planes, size, wavelet, J in ((192, 224, "db4", 3), (384, 512, "sym8", 5)):
        fold = P.get_plan(2, (size, size), J, wavelet, "reflect", dev)
        axis = P.get_plan(2, (size, size), J, wavelet, "reflect", dev, generic=True)
        c = torch.randn(planes * fold.coeff_numel, device=dev, generator=gen)
        gx_f = torch.empty((planes, size, size), device=dev)
        gx_a = torch.empty_like(gx_f)
        rec = torch.empty((1, planes) + fold.rec_shape, device=dev)
        emit("geometry: %d planes of %d^2, %s J=%d, reflect; routes %s / %s; plan: %s"
             % (planes, size, wavelet, J, fold.wavedec_adjoint_routes, axis.wavedec_adjoint_routes, fold.routes))
        f_fold = lambda: fold.wavedec_adjoint(c, planes, out=gx_f)
        f_axis = lambda: axis.wavedec_adjoint(c, planes, out=gx_a)
        f_rec = lambda: fold.waverec(c, planes, out=rec)
        f_fold(), f_axis()
        emit("  fold vs axis: max |diff| %.3g of max |axis| %.3g"
             % (float((gx_f - gx_a).abs().max()), float(gx_a.abs().max())))
        kernel_rows(records_of(P, f_fold, a.reps), "fold", a.reps)
        kernel_rows(records_of(P, f_axis, a.reps), "axis", a.reps)
        tf, ta, tr = interleaved([f_fold, f_axis, f_rec], a.rounds)
        emit("  whole calls, %d interleaved rounds: fold %s; axis %s; wam_waverec %s; axis / fold %.2fx; "
             "fold / wam_waverec %.2fx" % (a.rounds, fmt(tf), fmt(ta), fmt(tr), np.median(ta) / np.median(tf),
                                            np.median(tf) / np.median(tr)))
        del c, gx_f, gx_a, rec
        torch.cuda.empty_cache()

    for ndim, batch, shape, wavelet, J in ((1, 256, (80000,), "db6", 5), (3, 16, (128, 128, 128), "haar", 2)):
        plan = P.get_plan(ndim, shape, J, wavelet, "reflect", dev)
        c = torch.randn(batch * plan.coeff_numel, device=dev, generator=gen)
        gx = torch.empty((batch,) + shape, device=dev)
        rec = torch.empty((1, batch) + plan.rec_shape, device=dev)
        emit("geometry: %d items of %s, %s J=%d, reflect; routes %s; plan: %s"
             % (batch, "x".join(map(str, shape)), wavelet, J, plan.wavedec_adjoint_routes, plan.routes))
        f_adj = lambda: plan.wavedec_adjoint(c, batch, out=gx)
        f_rec = lambda: plan.waverec(c, batch, out=rec)
        kernel_rows(records_of(P, f_adj, a.reps), "axis", a.reps)
        ta, tr = interleaved([f_adj, f_rec], a.rounds)
        emit("  whole calls, %d interleaved rounds: axis %s; wam_waverec %s; axis / wam_waverec %.2fx"
             % (a.rounds, fmt(ta), fmt(tr), np.median(ta) / np.median(tr)))
        del c, gx, rec
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
