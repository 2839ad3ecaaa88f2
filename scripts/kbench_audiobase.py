"""The tiled Grad-CAM route (wam_amd/csrc/cam_tiled.hip) at the audio shapes it was written for, and beside
the LDS kernel at the shape that kernel was measured at.

Three measurements, each 20 interleaved rounds in one process (the order of the paths rotates), device
events around each whole path, medians:
  1. wam_cam_maps_tiled against a vectorised torch form of the same arithmetic (float32) at
     8 x 16 x 157x128 -> 157x128 (the c3 mel, a first-block layer of the audio CNN);
  2. the same at 8 x 16 x 431x128 -> 431x128 (the reference's ESC-50 mel);
  3. wam_cam_maps_tiled against wam_cam_maps (and torch) at 64 x 2048 x 7x7 -> 224^2, inside the LDS
     bound, where profiles/baselines_kbench.txt has wam_cam_maps at 0.44-0.62x of torch.
The three kernels' own times come from the library's launch records. The figures are recorded
(profiles/audiobase_kbench.txt), not gated; wam_amd.baselines.cam_maps keeps in-bound shapes on wam_cam_maps.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scripts.kbench_baselines import interleaved, kernel_rows  # noqa: E402

KERNELS = ("k_cam_weight_parts", "k_cam_plane", "k_cam_resize", "k_cam_maps")


def cam_torch(act, grad, pp, size):
    if pp:
        w = (grad.clamp(min=0) * act).sum(dim=(2, 3)) / (act.sum(dim=(2, 3)) + 1e-8)
    else:
        w = grad.mean(dim=(2, 3))
    cam = F.relu((w[:, :, None, None] * act).sum(dim=1))
    cam = cam - cam.amin(dim=(1, 2), keepdim=True)
    cam = cam / cam.amax(dim=(1, 2), keepdim=True)
    return F.interpolate(cam[:, None], size=size, mode="bilinear", align_corners=False)[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_audiobase needs a HIP device"
    from wam_amd.baselines import CAM_LDS_CAP, cam_maps, cam_maps_tiled
    from wam_amd.plan import timing_drain, timing_enable

    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    for N, K, h, w, size in ((8, 16, 157, 128, (157, 128)), (8, 16, 431, 128, (431, 128)), (64, 2048, 7, 7, (224, 224))):
        act = torch.as_tensor(rs.uniform(0.0, 1.0, size=(N, K, h, w)).astype(np.float32)).to(dev)
        grad = torch.as_tensor(np.abs(rs.standard_normal((N, K, h, w))).astype(np.float32)).to(dev)
        in_cap = 8 * (K + h * w + 1040) <= CAM_LDS_CAP
        for pp in (False, True):
            paths = {"tiled": lambda: cam_maps_tiled(act, grad, pp, size), "torch": lambda: cam_torch(act, grad, pp, size)}
            if in_cap:
                paths["lds"] = lambda: cam_maps(act, grad, pp, size)
            err = float((paths["tiled"]() - paths["torch"]()).abs().max())
            res = interleaved(paths, a.rounds)
            what = "%s, %d x %d x %dx%d -> %dx%d" % ("Grad-CAM++" if pp else "Grad-CAM", N, K, h, w, size[0], size[1])
            for k, (med, lo, hi) in res.items():
                print("%s, %d interleaved rounds: %-6s median %.3f ms (min %.3f, max %.3f); torch / this = %.2fx"
                      % (what, a.rounds, k, med, lo, hi, res["torch"][0] / med))
            print("%s: max |tiled - torch| %.2e" % (what, err))
        timing_enable(True)
        for _ in range(10):
            cam_maps_tiled(act, grad, False, size)
            if in_cap:
                cam_maps(act, grad, False, size)
        torch.cuda.synchronize()
        kernel_rows(timing_drain(), KERNELS if in_cap else KERNELS[:3])
        timing_enable(False)


if __name__ == "__main__":
    main()
