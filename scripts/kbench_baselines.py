"""The pixel-domain baseline kernels (wam_amd/csrc/baselines2d.hip) at EvalImageBaselines' working
geometry, each against the composition of entries the library already had, and one ``insertion`` call
against the CPU restatement (tests/baselines_ref.py).

Four measurements:
  1. wam_rank_mask_pixels (8 images x 3 x 224^2, n_iter 128 -> 1032 model inputs) against
     wam_rank_masks + a torch multiply + wam_quantize_normalize per image (masks and masked floats stored
     in memory). Outputs asserted bit-equal, then interleaved rounds in one process (the order of the paths rotates) with device
     events around each whole path; medians, and the achieved bytes/s of the fused path on its
     algorithmic bytes (read 4 (C + 1) P per set, write 4 M C P) beside the 8 TB/s peak and the 6.3 TB/s
     copy ceiling. --variant PATH adds a second build of the library (streaming stores for `out`) to
     the same rounds. The two kernels' own times come from the library's launch records.
  2. wam_cell_mask_pixels (512 masks, grid 28, one 3 x 224^2 image) against wam_upsample_masks + multiply
     + wam_quantize_normalize, measured the same way.
  3. wam_cam_maps (64 images x 2048 x 7 x 7 -> 224^2) against a vectorised torch form of the same
     arithmetic (float32), and against the reference's literal per-channel loop on one image, scaled.
  4. end to end: EvalImageBaselines.insertion (8 images, n_iter 128, TinySmooth2D, injected explanations)
     on the device against the CPU restatement on --cpu-images images, scaled.
"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK, COPY_CEILING = 8e12, 6.3e12


def interleaved(paths, rounds, warm=3):
    """Median / min / max ms of each path over `rounds` rounds; the order rotates from round to round
    (A B C, B C A, ...), so that no path always runs behind the same neighbour's write-back."""
    for _ in range(warm):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(paths) + 1)]
    names = list(paths)
    ts = {k: [] for k in names}
    for r in range(rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        ev[0].record()
        for i, k in enumerate(order):
            paths[k]()
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i, k in enumerate(order):
            ts[k].append(ev[i].elapsed_time(ev[i + 1]))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ts.items()}


def report(what, res, fused_bytes, composed_bytes, rounds):
    base = res["composition"][0]
    for k, (med, lo, hi) in res.items():
        extra = ""
        if k != "composition":
            rate = fused_bytes / (med * 1e-3)
            extra = "; %.0f GB/s on %.1f MB algorithmic = %.1f %% of 8 TB/s, %.1f %% of the 6.3 TB/s copy ceiling; " \
                    "composition / this = %.2fx" % (rate / 1e9, fused_bytes / 1e6, 100 * rate / HBM_PEAK,
                                                    100 * rate / COPY_CEILING, base / med)
        print("%s, %d interleaved rounds: %-11s median %.3f ms (min %.3f, max %.3f)%s"
              % (what, rounds, k, med, lo, hi, extra))
    print("%s: bytes moved by the composition %.1f MB = %.2fx the fused path's" % (what, composed_bytes / 1e6,
                                                                                   composed_bytes / fused_bytes))


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
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--n-iter", type=int, default=128)
    ap.add_argument("--masks", type=int, default=512)
    ap.add_argument("--grid", type=int, default=28)
    ap.add_argument("--cam-images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cpu-images", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the CPU restatement")
    ap.add_argument("--variant", default=None, help="a second libwam_hip.so build to time in the same rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_baselines needs a HIP device"
    import testmodels
    from tests import baselines_ref as R
    from tests.golden.imgbase_cases import distinct_positive
    from wam_amd import _lib
    from wam_amd._lib import c_f32, check, lib, ptr, stream_of
    from wam_amd.baselines import EvalImageBaselines, cam_maps
    from wam_amd.evalcore import cell_map, descending_ranks
    from wam_amd.evaluation import IMAGENET_MEAN, IMAGENET_STD
    from wam_amd.plan import timing_drain, timing_enable

    dev = torch.device("cuda", 0)
    st = stream_of(dev)
    N, S, n_iter = a.images, a.size, a.n_iter
    P, M = S * S, n_iter + 1
    rs = np.random.RandomState(0)
    imgs = torch.as_tensor(rs.uniform(size=(N, 3, P)).astype(np.float32)).to(dev)
    expl = distinct_positive(rs, (N, P))
    rank = descending_ranks(expl, dev, "stable")
    mean, std = (c_f32 * 3)(*IMAGENET_MEAN), (c_f32 * 3)(*IMAGENET_STD)
    variant = None
    if a.variant:
        variant = ctypes.CDLL(a.variant)
        for name in ("wam_rank_mask_pixels", "wam_cell_mask_pixels"):
            getattr(variant, name).restype = _lib._SIGS[name][0]
            getattr(variant, name).argtypes = _lib._SIGS[name][1]
    print("geometry: %d images x 3 x %d^2, n_iter %d -> %d model inputs; %d superpixel masks at grid %d; %d CAMs"
          % (N, S, n_iter, N * M, a.masks, a.grid, a.cam_images))

    # ---- 1. ranking -> model inputs
    out_f = torch.empty((N * M, 3, P), dtype=torch.float32, device=dev)
    out_v = torch.empty_like(out_f)
    out_c = torch.empty_like(out_f)
    ws = torch.empty(int(lib.wam_rank_mask_pixels_ws_bytes(N, n_iter)) // 4, dtype=torch.float32, device=dev)
    n_comp = int(P / n_iter)

    def rank_fused(L=lib, o=out_f):
        check(L.wam_rank_mask_pixels(N, 3, P, ptr(imgs), ptr(rank), n_iter, n_comp, 0, mean, std, None, None, ptr(o),
                                     ptr(ws), st))

    masks = torch.empty((M, P), dtype=torch.float32, device=dev)

    def rank_composed():
        for s in range(N):
            check(lib.wam_rank_masks(n_iter, n_comp, P, ptr(rank[s]), 0, ptr(masks), st))
            masked = masks[:, None, :] * imgs[s][None]
            check(lib.wam_quantize_normalize(M, 3, P, ptr(masked), mean, std, ptr(out_c[s * M:(s + 1) * M]), st))

    rank_fused(), rank_composed()
    same = torch.equal(out_f, out_c)
    paths = {"fused": rank_fused, "composition": rank_composed}
    if variant is not None:
        rank_fused(variant, out_v)
        same = same and torch.equal(out_v, out_c)
        paths = {"fused": rank_fused, "nt-stores": lambda: rank_fused(variant, out_v), "composition": rank_composed}
    print("wam_rank_mask_pixels and the composition bit-equal: %s" % same)
    assert same
    fused_b = N * (4.0 * 4 * P + 4.0 * M * 3 * P)
    # composition per image: masks written and read, image read, masked floats written and read twice, out written
    comp_b = N * (4.0 * P + 4.0 * M * P * 2 + 4.0 * 3 * P + 4.0 * M * 3 * P * 4)
    report("ranking to model inputs", interleaved(paths, a.rounds), fused_b, comp_b, a.rounds)
    timing_enable(True)
    timing_drain()
    for _ in range(a.rounds):
        rank_fused()
    torch.cuda.synchronize()
    kernel_rows(timing_drain(), ["k_rank_extrema", "k_rank_scan", "k_rank_mask_pixels"])
    timing_enable(False)
    del out_v, out_c, masks

    # ---- 2. superpixel masks -> model inputs
    n, g = a.masks, a.grid
    cell = cell_map(g, (S, S), dev)
    grid = torch.as_tensor(rs.uniform(size=(n, g * g)).astype(np.float32)).to(dev)
    img = imgs[0].contiguous()
    out_f = torch.empty((n, 3, P), dtype=torch.float32, device=dev)
    out_v = torch.empty_like(out_f)
    out_c = torch.empty_like(out_f)
    up = torch.empty((n, P), dtype=torch.float32, device=dev)

    def cell_fused(L=lib, o=out_f):
        check(L.wam_cell_mask_pixels(3, P, ptr(img), n, g * g, ptr(grid), ptr(cell), mean, std, None, None, ptr(o), st))

    def cell_composed():
        check(lib.wam_upsample_masks(n, g * g, ptr(grid), P, ptr(cell), ptr(up), st))
        masked = up[:, None, :] * img[None]
        check(lib.wam_quantize_normalize(n, 3, P, ptr(masked), mean, std, ptr(out_c), st))

    cell_fused(), cell_composed()
    same = torch.equal(out_f, out_c)
    paths = {"fused": cell_fused, "composition": cell_composed}
    if variant is not None:
        cell_fused(variant, out_v)
        same = same and torch.equal(out_v, out_c)
        paths = {"fused": cell_fused, "nt-stores": lambda: cell_fused(variant, out_v), "composition": cell_composed}
    print("wam_cell_mask_pixels and the composition bit-equal: %s" % same)
    assert same
    fused_b = 4.0 * 4 * P + 4.0 * n * g * g + 4.0 * n * 3 * P
    comp_b = 4.0 * n * g * g + 4.0 * P + 4.0 * n * P * 2 + 4.0 * 3 * P + 4.0 * n * 3 * P * 4
    report("superpixel masks to model inputs", interleaved(paths, a.rounds), fused_b, comp_b, a.rounds)
    del out_f, out_v, out_c, up

    # ---- 3. CAMs
    NC, K, h = a.cam_images, 2048, 7
    act = torch.as_tensor(rs.uniform(0, 1, size=(NC, K, h, h)).astype(np.float32)).to(dev)
    grad = torch.as_tensor(rs.standard_normal((NC, K, h, h)).astype(np.float32)).to(dev)

    def cam_torch(pp):
        if pp:
            w = (grad.clamp(min=0) * act).sum(dim=(2, 3)) / (act.sum(dim=(2, 3)) + 1e-8)
        else:
            w = grad.mean(dim=(2, 3))
        cam = F.relu((w[:, :, None, None] * act).sum(dim=1))
        cam = cam - cam.amin(dim=(1, 2), keepdim=True)
        cam = cam / cam.amax(dim=(1, 2), keepdim=True)
        return F.interpolate(cam[:, None], size=(S, S), mode="bilinear", align_corners=False)[:, 0]

    def cam_loop(i):  # src/evaluation_helpers.py:206-224 on one image
        weights = torch.mean(grad[i], dim=[1, 2])
        cam = torch.zeros(act.shape[2:], dtype=torch.float32, device=dev)
        for j, w in enumerate(weights):
            cam += w * act[i, j, :, :]
        cam = F.relu(cam)
        cam = cam - cam.min()
        cam = cam / cam.max()
        return F.interpolate(cam[None, None], size=(S, S), mode="bilinear", align_corners=False)[0, 0]

    for pp in (False, True):
        k, t = cam_maps(act, grad, pp, (S, S)), cam_torch(pp)
        assert torch.equal(k.isnan(), t.isnan())   # a CAM that is nowhere positive is NaN in both
        d = float(torch.nan_to_num(k - t).abs().max())
        res = interleaved({"kernel": lambda: cam_maps(act, grad, pp, (S, S)), "torch": lambda: cam_torch(pp)}, a.rounds)
        print("%s, %d images x %d x %dx%d -> %d^2, %d interleaved rounds: wam_cam_maps median %.3f ms (min %.3f, max "
              "%.3f); vectorised torch median %.3f ms (min %.3f, max %.3f); ratio %.2fx; max |kernel - torch| %.2e"
              % ("Grad-CAM++" if pp else "Grad-CAM", NC, K, h, h, S, a.rounds, *res["kernel"], *res["torch"],
                 res["torch"][0] / res["kernel"][0], d))
    cam_loop(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cam_loop(1)
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t0
    print("the reference's per-channel loop (%d launches) on one image: %.1f ms, scaled to %d images %.2f s"
          % (K, 1e3 * t_loop, NC, t_loop * NC))

    # ---- 4. end to end
    model = testmodels.TinySmooth2D()
    x = torch.as_tensor(rs.uniform(size=(N, 3, S, S)).astype(np.float32))
    y = [int(v) for v in rs.randint(0, 10, N)]
    expl = expl.reshape(N, S, S)
    ev = EvalImageBaselines("saliency", testmodels.TinySmooth2D().to(dev))
    ev.explanations = expl
    scores = ev.insertion(x, y, n_iter=n_iter)   # warm-up: MIOpen's algorithm search
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        scores = ev.insertion(x, y, n_iter=n_iter)
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / a.calls
    torch.set_num_threads(a.threads)
    nc = max(1, min(a.cpu_images, N))
    t0 = time.perf_counter()
    ref_scores, _ = R.evaluate_auc(model, expl[:nc], x[:nc], y[:nc], "insertion", n_iter=n_iter)
    t_cpu = (time.perf_counter() - t0) * N / nc
    print("end to end insertion, %d images, n_iter %d, TinySmooth2D: device %.1f ms / call (mean of %d); CPU "
          "restatement %.2f s (measured on %d images on %d threads, scaled to %d); ratio %.0fx; max |d score| on the "
          "compared images %.2e" % (N, n_iter, 1e3 * t_dev, a.calls, t_cpu, nc, a.threads, N, t_cpu / t_dev,
                                    float(np.abs(np.array(scores[:nc]) - np.array(ref_scores)).max())))


if __name__ == "__main__":
    main()
