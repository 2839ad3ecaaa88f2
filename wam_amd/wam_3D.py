"""WAM for volumes on MI355X: drop-in for the reference's ``lib/wam_3D.py`` voxel path.

``BaseWAM3D`` (lib/wam_3D.py:88-245, voxels) and ``WaveletAttribution3D`` (:501-660) with the
same constructor arguments, call signatures, float32 cube outputs and side attributes
(``coeffs``, ``grads``, ``input_size``). All volumes of a batch (and several noise samples / IG
steps) are transformed in one launch instead of the reference's per-volume Python loop
(:193); the |grad| cube packing (``refactor``) is a gather map over the band-major gradients;
the reference's in-loop averaging of ``smooth`` (:585-587, result = sum_s cube_s * n^-(n-s)) is
reproduced exactly. Point clouds are not implemented in the reference either (:381-383): the entry
prints 'Not implemented yet' as there; its unreachable ``evaluate_point_clouds`` (:247-358) is
provided on the GPU 1D kernels. Post-processing: ``visualize`` (:662-719) is
the k_vis3d_* kernels; ``filter_voxels`` (:439-495) thresholds on the device and reconstructs with
the 3D synthesis kernels.
Build-only kwargs: noise, frame ('legacy' keeps the inner 16^3 refactor size of IG), sample_batch,
autocast_dtype, dist.
"""
import numpy as np
import torch

from . import frames
from .constants import KEYS3
from .engine import (LegacyNoise, Shard, auto_group, chunks, ig_weights, input_gradient, legacy3d_weights,
                     model_device, param_grad_sum, require_gpu_device, trainable_params)
from ._lib import check, lib, ptr, stream_of
from .profiling import phase
from .plan import (CAP_NOISY_WAVEDEC, cube_accumulate, cube_moments, get_plan, item_sigma, moments_finish, noise_add,
                   subband_maps)


class BaseWAM3D:
    def __init__(self, model, wavelet="haar", J=1, approx_coeffs=False, device=None, mode="symmetric",
                 instance="voxels", normalize=True, EPS=0.451, *, frame="legacy", autocast_dtype=None):
        self.wavelet = wavelet
        self.J = J
        self.approx_coeffs = approx_coeffs
        self.mode = mode
        self.instance = instance
        self.EPS = EPS
        self.normalize = normalize
        self.input_size = None
        if device is not None:
            model = model.to(device)
            self.model = model
            self.device = device
        else:
            self.model = model
            self.device = next(model.parameters()).device
        self.frame = frame
        self.autocast_dtype = autocast_dtype
        self._coeffs_src = None
        self._coeffs = None
        self._grads_src = None
        self._grad_lists = None

    @property
    def _dev(self):
        return require_gpu_device(model_device(self.model, self.device))

    # ------------------------------------------------------------------ side attribute .coeffs
    @property
    def coeffs(self):
        if self._coeffs is None and self._coeffs_src is not None:
            self._coeffs = self._item_lists(*self._coeffs_src)
        return self._coeffs

    @coeffs.setter
    def coeffs(self, v):
        self._coeffs = v

    @staticmethod
    def _item_lists(plan, flat, items, first, n, c):
        views = [v[first * c:(first + n) * c].detach().cpu().numpy() for v in plan.split(flat, items)]
        out = []
        for k in range(n):
            sq = [views[b][k * c:(k + 1) * c].squeeze() for b in range(plan.nbands)]
            out.append([sq[0]] + [{key: sq[1 + 7 * lv + j] for j, key in enumerate(KEYS3)}
                                  for lv in range(plan.levels)])
        return out

    @property
    def grads(self):
        """Per-volume coefficient gradients of the last evaluate_voxels pass (the reference's
        detached_grads, lib/wam_3D.py:241; filter_voxels reads them); WaveletAttribution3D
        overwrites it with the |grad| cube, as the reference does (:589)."""
        if self._grad_lists is None and self._grads_src is not None:
            self._grad_lists = self._item_lists(*self._grads_src)
        return self._grad_lists

    @grads.setter
    def grads(self, v):
        self._grad_lists = v
        self._grads_src = None

    def filter_voxels(self, normalized=True):
        """lib/wam_3D.py:439-495: keep the coefficients whose normalised gradient passes EPS and
        reconstruct: approximation x min-max-normalised gradient; details x (|g| / max(g) >= EPS)
        (max of the SIGNED gradient, as the reference). Masks on the device, waverec3 on the 3D
        synthesis kernels; returns [N, D, H, W] float32 (one reconstruction per volume; the
        reference hands ptwt.waverec3 squeezed 3-D coefficients)."""
        grads, coeffs = self.grads, self.coeffs
        if grads is None or coeffs is None:
            raise AttributeError("filter_voxels needs the coefficient gradients and coefficients of a pass")
        out = []
        dev = self._dev
        for grad, coeff in zip(grads, coeffs):
            if not isinstance(grad, (list, tuple)):
                raise AttributeError("'numpy.ndarray' object has no attribute 'keys'")  # the |grad| cube
            g0 = torch.as_tensor(np.asarray(grad[0]), dtype=torch.float32, device=dev)
            ag = (g0 - g0.min()) / (g0 - g0.min()).max()
            bands = [torch.as_tensor(np.asarray(coeff[0]), dtype=torch.float32, device=dev) * ag]
            for dg_l, dc_l in zip(grad[1:], coeff[1:]):
                for key in KEYS3:
                    dg = torch.as_tensor(np.asarray(dg_l[key]), dtype=torch.float32, device=dev)
                    dc = torch.as_tensor(np.asarray(dc_l[key]), dtype=torch.float32, device=dev)
                    bands.append(dc * ((dg.abs() / dg.max()) >= self.EPS).float())
            from .filters import get_wavelet
            L = len(get_wavelet(self.wavelet).dec_lo)
            fin = bands[-1].shape
            plan = get_plan(3, tuple(2 * m + 2 - L if L > 2 else 2 * m for m in fin), len(grad) - 1, self.wavelet,
                            self.mode, dev)
            flat = torch.cat([b.reshape(-1) for b in bands])
            out.append(plan.waverec(flat, 1)[0][0].cpu().numpy())
        return np.array(out)

    def evaluate_point_clouds(self, x, y, permute):
        """lib/wam_3D.py:247-358 (unreachable from __call__ in the reference, which prints 'Not
        implemented yet'): 1D wavedec of the flattened [B, N*3] coordinates, waverec, the model on
        the [B, N, 3] reconstruction (a tuple-returning point net when permute is given), the
        diag-mean loss, coefficient gradients by the adjoint. Returns (coeffs, coeffs) as the
        reference does (:358); the gradients are kept in self.point_grads."""
        dev = self._dev
        x = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
        self.batch_size, self.shape_size = x.shape[0], x.shape[1]
        self.input = x.cpu().numpy()
        flat_x = x.view(x.shape[0], -1)
        plan = get_plan(1, (flat_x.shape[1],), self.J, self.wavelet, "reflect", dev)  # ptwt.wavedec's default mode
        z = plan.wavedec(flat_x)
        rec = plan.waverec(z, x.shape[0])[0][:, :flat_x.shape[1]].reshape(x.shape)
        leaf = rec.detach().requires_grad_(True)
        with torch.enable_grad():
            out = self.model(leaf.permute(permute)) if permute is not None else self.model(leaf)
            if isinstance(out, tuple):
                out = out[0]
            loss = torch.diag(out[:, y]).mean()
            (g,) = torch.autograd.grad(loss, leaf)
        g_full = torch.zeros((x.shape[0],) + plan.rec_shape, device=dev)
        g_full[:, :flat_x.shape[1]] = g.reshape(x.shape[0], -1)
        cg = plan.adjoint(g_full)
        coeffs = [v.cpu().numpy() for v in plan.split(z, x.shape[0])]
        self.point_grads = [v.cpu().numpy() for v in plan.split(cg, x.shape[0])]
        return coeffs, coeffs

    def refactor(self, coeffs, input_size=16):
        """lib/wam_3D.py:127-166 on host coefficient lists (API compatibility)."""
        if self.input_size is None:
            self.input_size = input_size
        S = self.input_size
        out = np.empty((len(coeffs), S, S, S), dtype=np.float32)
        idx = [int(S / 2 ** j) for j in range(self.J + 1)][::-1]
        idx.insert(0, 0)
        for k, c in enumerate(coeffs):
            for i in range(self.J + 1):
                s, e = idx[i], idx[i + 1]
                if s == 0:
                    out[k, :e, :e, :e] = np.abs(c[i])
                else:
                    lv = c[i]
                    out[k, s:e, s:e, s:e] = np.abs(lv["ddd"])
                    out[k, :s, :s, s:e] = np.abs(lv["aad"])
                    out[k, :s, s:e, :s] = np.abs(lv["ada"])
                    out[k, :s, s:e, s:e] = np.abs(lv["add"])
                    out[k, s:e, :s, :s] = np.abs(lv["daa"])
                    out[k, s:e, :s, s:e] = np.abs(lv["dad"])
                    out[k, s:e, s:e, :s] = np.abs(lv["dda"])
        return out

    # ------------------------------------------------------------------ core
    def _check_channels(self, c, s):
        if c != 1:
            # the reference squeezes [C, s, s, s] and fails to place it in the cube
            raise ValueError("could not broadcast input array from shape (%d,%d,%d,%d) into shape (%d,%d,%d)"
                             % (c, s, s, s, s, s, s))

    def _grads(self, plan, flat, items, y, groups, n, c):
        rec = plan.waverec(flat, items)[0].view((groups * n, c) + plan.rec_shape)
        if y is None:
            g = input_gradient(self.model, rec.unsqueeze(0), None, 1, 1, self.autocast_dtype, y_none_mean=True)[0]
        else:
            g = input_gradient(self.model, rec, y, groups, n, self.autocast_dtype)
        return plan.adjoint(g.view((items,) + plan.rec_shape))

    def _cube_from_grads(self, plan, cg, items, groups, n, input_size, acc, mode, n_total=1.0, weights=None,
                         prev=None, k0=0):
        maps, _ = subband_maps(plan, cg, groups, n, 1, want_max=False)  # the cube is not normalised
        src = frames.cube_map(plan, input_size, cg.device)
        cube_accumulate(groups, k0, n, src, maps, plan.coeff_numel, mode, n_total, acc, prev=prev, weights=weights)

    def evaluate_voxels(self, x, y, shape=True):
        """lib/wam_3D.py:168-245: one gradient pass, returns the |grad| cube [N, S, S, S] float32."""
        dev = self._dev
        if shape:
            x = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
            self.input_size = x.shape[-1]
            n, c = x.shape[:2]
            sp = tuple(x.shape[2:])
            plan = get_plan(3, sp, self.J, self.wavelet, self.mode, dev)
            flat = plan.wavedec(x.view((n * c,) + sp))
        else:
            items = list(x)
            n = len(items)
            c = items[0][0].shape[0]
            from .filters import get_wavelet
            L = len(get_wavelet(self.wavelet).dec_lo)
            fin = next(iter(items[0][-1].values())).shape[-3:]
            plan = get_plan(3, tuple(2 * m + 2 - L for m in fin), len(items[0]) - 1, self.wavelet, self.mode, dev)
            bands = []
            for b in range(plan.nbands):
                if b == 0:
                    bands.append(torch.stack([it[0] for it in items]))
                else:
                    lv, j = divmod(b - 1, 7)
                    bands.append(torch.stack([it[1 + lv][KEYS3[j]] for it in items]))
            flat = torch.cat([t.detach().to(dev, torch.float32).reshape(-1) for t in bands])
        self._check_channels(c, plan.band_shapes[0][0])
        cg = self._grads(plan, flat, n * c, y, 1, n, c)
        self._coeffs_src = (plan, flat, n * c, 0, n, c)
        self._coeffs = None
        self._grads_src = (plan, cg, n * c, 0, n, c)
        self._grad_lists = None
        S = self.input_size if self.input_size is not None else 16
        if self.input_size is None:
            self.input_size = S
        acc = torch.zeros(n * S ** 3, dtype=torch.float32, device=dev)
        one = torch.ones(1, dtype=torch.float32, device=dev)
        self._cube_from_grads(plan, cg, n * c, 1, n, S, acc, 1, weights=one)
        return acc.view(n, S, S, S).cpu().numpy()

    def __call__(self, x, y=None, permute=None, shape=True):
        if self.instance == "voxels":
            return self.evaluate_voxels(x, y, shape=shape)
        elif self.instance == "point_clouds":
            print("Not implemented yet")


class WaveletAttribution3D(BaseWAM3D):
    def __init__(self, model, wavelet="haar", J=3, approx_coeffs=False, device=None, mode="symmetric",
                 instance="voxels", method="smooth", normalize=True, EPS=0.451, n_samples=25, stdev_spread=0.0001,
                 random_seed=42, *, noise="numpy", frame="legacy", sample_batch=None, autocast_dtype=None,
                 dist=None):
        super().__init__(model, wavelet=wavelet, J=J, approx_coeffs=approx_coeffs, device=device, mode=mode,
                         instance=instance, normalize=normalize, EPS=EPS, frame=frame,
                         autocast_dtype=autocast_dtype)
        self.n_samples = n_samples
        self.stdev_spread = stdev_spread
        self.random_seed = random_seed
        self.method = method
        if noise not in ("numpy", "philox"):
            raise ValueError("noise must be 'numpy' or 'philox'")
        self.noise = noise
        self.sample_batch = sample_batch
        self.dist = dist
        self.smooth_mean = None  # the plain mean cube of the last 'smooth_sq' / 'vargrad' call
        self.wam = BaseWAM3D(model, wavelet=wavelet, J=J, mode=mode, device=device, approx_coeffs=approx_coeffs,
                             instance=instance, normalize=normalize, EPS=EPS, frame=frame,
                             autocast_dtype=autocast_dtype)

    def smooth(self, x, y=None, permute=None, moment=None):
        """lib/wam_3D.py:550-591 (noise on channel 0 only; legacy in-loop averaging). moment
        (build-only): 'smooth_sq' / 'vargrad' = the mean square / the population variance of the
        per-sample |gradient| cubes over the noise samples (wam_cube_moments: sum and sum of squares
        in float64, one pass over the maps; float32 results). These use the PLAIN mean over the
        samples, not the reference's in-loop averaging of 'smooth' (weights n^-(n-s)); that plain mean
        of the same run is left in self.smooth_mean."""
        dev = self._dev
        x = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
        S = x.shape[-1]
        if self.input_size is None:
            self.input_size = S
        n, c = x.shape[:2]
        sp = tuple(x.shape[2:])
        vol = int(np.prod(sp))
        plan = get_plan(3, sp, self.J, self.wavelet, self.mode, dev)
        self._check_channels(c, plan.band_shapes[0][0])
        self.wam.input_size = S
        sigma = item_sigma(x, c * vol, vol, self.stdev_spread)
        shard = Shard(self.dist)
        s_lo, s_hi = shard.range(self.n_samples)
        group = 1 if y is None else auto_group(self.model, n, self.sample_batch, cap_items=32)
        legacy = None
        if self.noise == "numpy":
            legacy = LegacyNoise(sigma.cpu().numpy(), sp, self.random_seed, self.n_samples, dev)
        acc = torch.zeros(n * S ** 3, dtype=torch.float32 if moment is None else torch.float64, device=dev)
        acc_q = None if moment is None else torch.zeros_like(acc)
        ns = self.n_samples
        with param_grad_sum(trainable_params(self.model), shard):
            for s0, cnt in chunks(s_lo, s_hi, group):
                host = None
                if legacy is not None:
                    host = legacy.chunk(s0, cnt)  # [cnt, n, *sp]
                    if c > 1:  # the reference noises channel 0 only
                        full = torch.zeros((cnt, n, c) + sp, dtype=torch.float32, device=dev)
                        full[:, :, 0] = host
                        host = full
                with phase("noise+wavedec3"):
                    if host is None and c == 1 and plan.caps & CAP_NOISY_WAVEDEC:  # noise fused on the load
                        flat = plan.wavedec_noisy(x, sigma, cnt, n, 1, self.random_seed, s0)
                    else:
                        noisy = noise_add(x, sigma, cnt, n, c * vol, vol, seed=self.random_seed, sample_base=s0,
                                          host_noise=host)
                        flat = plan.wavedec(noisy.view((cnt * n * c,) + sp))
                with phase("waverec3+model+adjoint"):
                    cg = self._grads(plan, flat, cnt * n * c, y, cnt, n, c)
                if moment is not None:
                    maps, _ = subband_maps(plan, cg, cnt, n, 1, want_max=False)
                    cube_moments(cnt, n, frames.cube_map(plan, S, dev), maps, plan.coeff_numel, acc, acc_q)
                elif shard.world == 1:
                    self._cube_from_grads(plan, cg, cnt * n * c, cnt, n, S, acc, 0, n_total=float(ns))
                else:
                    w = torch.from_numpy(legacy3d_weights(s0, cnt, ns)).to(dev)
                    self._cube_from_grads(plan, cg, cnt * n * c, cnt, n, S, acc, 1, weights=w)
                self.wam._coeffs_src = (plan, flat, cnt * n * c, (cnt - 1) * n, n, c)
                self.wam._coeffs = None
        if legacy is not None:
            legacy.finish()
        with phase("collectives"):
            shard.all_reduce_sum(acc)
            if acc_q is not None:  # linear in the samples, like the sum
                shard.all_reduce_sum(acc_q)
        if moment is not None:
            self.smooth_mean = moments_finish(acc, acc_q, ns, "mean", torch.float32).view(n, S, S, S).cpu().numpy()
            acc = moments_finish(acc, acc_q, ns, moment, torch.float32)
        self._cube_dev = acc.view(n, S, S, S)
        out = self._cube_dev.cpu().numpy()
        self.grads = out
        return out

    def visualize(self):
        """lib/wam_3D.py:662-719 on the device: [N, J + 2, S, S, S] float32 -- per level the
        (approximation / six-orientation sum) block upsampled by scipy zoom order 1 and divided by
        its max, then the level sum divided by its batch max (wam_visualize3d)."""
        dev = self._dev
        cube = getattr(self, "_cube_dev", None)
        if cube is None or not isinstance(self.grads, np.ndarray) or cube.shape != self.grads.shape:
            cube = torch.as_tensor(np.ascontiguousarray(self.grads, dtype=np.float32)).to(dev)
        n, S = cube.shape[0], cube.shape[-1]
        out = torch.empty((n, self.J + 2, S, S, S), dtype=torch.float32, device=dev)
        scratch = torch.empty(n * (self.J + 1) + 1, dtype=torch.float32, device=dev)
        check(lib.wam_visualize3d(n, S, self.J, ptr(cube.contiguous()), ptr(out), ptr(scratch), stream_of(dev)))
        return out.cpu().numpy()

    def alter(self, alpha, coeffs):
        """lib/wam_3D.py:594-611."""
        out = []
        for coeff in coeffs:
            tmp = [coeff[0] * alpha]
            for lv in coeff[1:]:
                tmp.append({k: v * alpha for k, v in lv.items()})
            out.append(tmp)
        return out

    def intergrated_wam(self, x, y=None, permute=None):
        """lib/wam_3D.py:614-643."""
        dev = self._dev
        x = torch.as_tensor(x).detach().to(dev, torch.float32).contiguous()
        S = x.shape[-1]
        n, c = x.shape[:2]
        sp = tuple(x.shape[2:])
        plan = get_plan(3, sp, self.J, self.wavelet, self.mode, dev)
        self._check_channels(c, plan.band_shapes[0][0])
        if self.input_size is None:
            self.input_size = S
        # the reference's inner BaseWAM3D refactors with input_size 16 unless it saw shape=True first
        inner = self.wam.input_size if self.wam.input_size is not None else (16 if self.frame == "legacy" else S)
        if inner != S:
            s = plan.band_shapes[0][0]
            raise ValueError("could not broadcast input array from shape (%d,%d,%d) into shape (%d,%d,%d)"
                             % (s, s, s, int(inner / 2 ** self.J), int(inner / 2 ** self.J), int(inner / 2 ** self.J)))
        self.wam.input_size = inner
        z = plan.wavedec(x.view((n * c,) + sp))
        base = torch.zeros(n * S ** 3, dtype=torch.float32, device=dev)
        one = torch.ones(1, dtype=torch.float32, device=dev)
        self._cube_from_grads(plan, z, n * c, 1, n, S, base, 1, weights=one)
        alphas = np.linspace(0, 1, self.n_samples)
        shard = Shard(self.dist)
        k_lo, k_hi = shard.range(self.n_samples)
        group = 1 if y is None else auto_group(self.model, n, self.sample_batch, cap_items=32)
        acc = torch.zeros(n * S ** 3, dtype=torch.float32, device=dev)
        prev = torch.zeros_like(acc)
        with param_grad_sum(trainable_params(self.model), shard):
            for k0, cnt in chunks(k_lo, k_hi, group):
                img = plan.waverec(z, n * c, alphas=alphas[k0:k0 + cnt])
                if y is None:
                    g = input_gradient(self.model, img.view((cnt * n, c) + plan.rec_shape).unsqueeze(0), None, 1, 1,
                                       self.autocast_dtype, y_none_mean=True)[0]
                else:
                    g = input_gradient(self.model, img.view((cnt * n, c) + plan.rec_shape), y, cnt, n,
                                       self.autocast_dtype)
                cg = plan.adjoint(g.reshape((cnt * n * c,) + plan.rec_shape))
                if shard.world == 1:
                    self._cube_from_grads(plan, cg, cnt * n * c, cnt, n, S, acc, 2, prev=prev, k0=k0)
                else:
                    wk = torch.from_numpy(ig_weights(k0, cnt, self.n_samples)).to(dev)
                    self._cube_from_grads(plan, cg, cnt * n * c, cnt, n, S, acc, 1, weights=wk)
        shard.all_reduce_sum(acc)
        self._cube_dev = base.view(n, S, S, S) * acc.view(n, S, S, S)
        out = self._cube_dev.cpu().numpy()
        self.grads = out
        return out

    def __call__(self, x, y=None, permute=None):
        if self.method == "smooth":
            return self.smooth(x, y)
        elif self.method == "integratedgrad":
            return self.intergrated_wam(x, y)
        elif self.method in ("smooth_sq", "vargrad"):
            return self.smooth(x, y, moment=self.method)
