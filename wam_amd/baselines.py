"""Pixel-domain baselines on MI355X: the methods WAM is compared against, and their evaluation.

Drop-in for the reference's ``EvalImageBaselines`` (``src/evaluators.py:805-1180``) and the helpers
under it (``src/evaluation_helpers.py:72-357``: ``GradCAM``, ``GradCAMPlusPlus``, ``SmoothGrad``,
``generate_images_baseline``, ``reconstruct_images_baseline``), with captum-shaped ``Saliency`` and
``IntegratedGradients`` for the two methods the reference takes from captum. The explained model's
forward and backward stay in PyTorch; everything after them runs on the HIP kernels of
``wam_amd/csrc/baselines2d.hip``:

  ranking of the explanation --wam_rank_mask_pixels--> the quantised, normalised model inputs of all
  n_iter + 1 insertion (deletion) masks of several images (the masks and the masked float images never
  reach memory); superpixel grids --wam_cell_mask_pixels--> the same for mu-fidelity's masks;
  activations and gradients of the target layer --wam_cam_maps--> Grad-CAM(++) maps, one workgroup per
  image (--wam_cam_maps_tiled, ``csrc/cam_tiled.hip``--> where the layer's map is past that kernel's LDS
  bound: full-resolution layers); input gradients --wam_channel_mean--> the [N, H, W] maps of Saliency, Integrated Gradients
  (steps summed by wam_trapz_f32) and SmoothGrad (noise by wam_item_sigma + wam_noise_add).

Host work left: the ranking's ``tie_order='numpy'`` option, Python / numpy RNG draws (the reference's
own streams), the softmax on [rows, classes] logits, spearmanr on sample_size values.
"""
import numpy as np
import torch
from scipy.stats import spearmanr

from . import plan as _plan
from ._lib import check, lib, ptr, stream_of
from .evalcore import (cell_map, check_tie_order, class_curves, class_probs, compute_auc, descending_ranks,
                       generate_subsets, masked_sums, norm_consts, resize_default, show_images, softmax)

METHODS = ("gradcam", "gradcampp", "saliency", "integratedgrad", "smoothgrad")
# methods of the reference that need packages this project does not carry
_NEEDS = {"guided_backprop": "captum", "layercam": "pytorch-grad-cam (pytorch_grad_cam)", "lrp": "zennit",
          "srd": "the SRD authors' code (srd_pytorch)"}


def _device_of(model, device=None):
    if device is not None:
        model.to(device)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("wam_amd: the model must live on a CUDA (HIP) device; the baseline kernels run on the "
                           "GPU only")
    return dev


def _targets(y, dev):
    return torch.as_tensor(y).to(dev).long().reshape(-1)


def channel_mean(g, mult=None, absolute=False, acc=None):
    """wam_channel_mean: g [N, C, H, W] float32 (device) -> [N, H, W] float32, numpy's float32 mean over
    the channel axis of g (* mult) (absolute value); with ``acc`` (float64 [N, H, W]) the mean is added
    to it instead and ``acc`` is returned."""
    g = g.contiguous()
    N, C, H, W = g.shape
    if mult is not None:
        mult = mult.contiguous()
    out = None if acc is not None else torch.empty((N, H, W), dtype=torch.float32, device=g.device)
    check(lib.wam_channel_mean(N, C, H * W, ptr(g), ptr(mult), int(bool(absolute)), ptr(out), ptr(acc),
                               stream_of(g.device)))
    return acc if acc is not None else out


def _input_grads(model, x, target):
    """d sum_i out[i, target[i]] / dx (captum's per-sample selection), float32 [N, C, H, W]."""
    x = x.detach().requires_grad_(True)
    out = model(x)
    sel = out.gather(1, target[:, None]).sum()
    return torch.autograd.grad(sel, x)[0].float().contiguous()


# ------------------------------------------------------------------------------------ CAMs
class GradCAM:
    """src/evaluation_helpers.py:157-230. ``target_layer``: the module whose output is explained
    (e.g. ``model.layer4[-1]``). ``__call__(x, y)`` -> numpy float32 [N, H, W]. The forward hook is held
    only during a call (the reference leaves it on the model). A CAM that is nowhere positive is NaN
    everywhere, as in the reference (0 / 0)."""

    plus_plus = False

    def __init__(self, model, target_layer, device=None):
        if isinstance(target_layer, (list, tuple)) and len(target_layer) == 1:
            target_layer = target_layer[0]
        if not isinstance(target_layer, torch.nn.Module):
            raise TypeError("target_layer must be a torch.nn.Module of the model")
        self.target_layer = target_layer
        self.model = model
        self.device = _device_of(model, device)
        self.model.eval()

    def forward(self, x):
        return self.model(x)

    def layer_tensors(self, x, y):
        """(activations, gradients) of the target layer, [N, K, h, w] float32 each, for the class scores
        out[i, y[i]]."""
        x = torch.as_tensor(x).detach().to(self.device, torch.float32).requires_grad_(True)
        target = _targets(y, self.device)
        kept = []
        hook = self.target_layer.register_forward_hook(lambda mod, inp, out: kept.append(out))
        try:
            out = self.forward(x)
        finally:
            hook.remove()
        if not kept or not isinstance(kept[-1], torch.Tensor) or kept[-1].dim() != 4:
            raise RuntimeError("GradCAM: the target layer must produce one [N, K, h, w] tensor in the forward pass")
        act = kept[-1]
        grad = torch.autograd.grad(out.gather(1, target[:, None]).sum(), act)[0]
        return act.detach().float().contiguous(), grad.float().contiguous()

    def __call__(self, input_images, target_classes):
        act, grad = self.layer_tensors(input_images, target_classes)
        return cam_maps(act, grad, self.plus_plus, tuple(input_images.shape[2:])).cpu().numpy()


class GradCAMPlusPlus(GradCAM):
    """src/evaluation_helpers.py:72-152: weights sum(max(grad, 0) * act) / (sum(act) + 1e-8), the
    reference's formula (not the paper's)."""

    plus_plus = True


CAM_LDS_CAP = 160 * 1024  # wam_cam_maps holds 8 * (K + h * w + 1040) bytes in one workgroup's LDS


def cam_maps(act, grad, plus_plus, size):
    """act, grad [N, K, h, w] float32 (device) -> [N, size[0], size[1]] float32: wam_cam_maps while the
    layer's map fits its LDS bound, wam_cam_maps_tiled (the plane in a workspace) above it."""
    N, K, h, w = act.shape
    if 8 * (K + h * w + 1040) > CAM_LDS_CAP:
        return cam_maps_tiled(act, grad, plus_plus, size)
    out = torch.empty((N, size[0], size[1]), dtype=torch.float32, device=act.device)
    check(lib.wam_cam_maps(N, K, h, w, ptr(act), ptr(grad), int(bool(plus_plus)), size[0], size[1], ptr(out),
                           stream_of(act.device)))
    return out


def cam_maps_tiled(act, grad, plus_plus, size):
    """wam_cam_maps_tiled: the same maps for any K and h * w."""
    N, K, h, w = act.shape
    out = torch.empty((N, size[0], size[1]), dtype=torch.float32, device=act.device)
    nbytes = int(lib.wam_cam_maps_tiled_ws_bytes(N, K, h, w))
    ws = torch.empty(max(nbytes, 0) // 8, dtype=torch.float64, device=act.device)
    check(lib.wam_cam_maps_tiled(N, K, h, w, ptr(act), ptr(grad), int(bool(plus_plus)), size[0], size[1], ptr(out),
                                 ptr(ws), nbytes, stream_of(act.device)))
    return out


# ------------------------------------------------------------------------------------ gradients
class SmoothGrad:
    """src/evaluation_helpers.py:234-320: the mean over ``n_samples`` noisy copies of the float32
    channel mean of d mean_i out[i, y[i]] / dx, numpy float64 [N, H, W]. The noise sigma_i =
    stdev_spread * (max - min) of image i is drawn on the device (wam_item_sigma + wam_noise_add,
    Philox keyed by ``random_seed``: sample s of a call is stream sample s); the reference's
    torch.normal stream is unseeded, so there is no stream to reproduce."""

    def __init__(self, model, n_samples=50, stdev_spread=0.25, random_seed=42, device=None):
        self.model = model
        self.n_samples = n_samples
        self.stdev_spread = stdev_spread
        self.random_seed = random_seed
        self.device = _device_of(model, device)

    def noisy(self, x, sample):
        """x + sigma * N(0, 1) of stream sample ``sample``: [N, C, H, W] float32 on the device."""
        N, item = x.shape[0], x[0].numel()
        sigma = _plan.item_sigma(x, item, item, self.stdev_spread)
        return _plan.noise_add(x, sigma, 1, N, item, item, seed=self.random_seed, sample_base=sample).view(x.shape)

    def compute_gradients(self, x, y, acc=None):
        """Channel mean of the gradient of diag(out[:, y]).mean() at x (device, [N, H, W] float32), or
        added into ``acc`` (float64)."""
        x = x.detach().requires_grad_(True)
        output = self.model(x)
        loss = torch.diag(output[:, y]).mean()
        return channel_mean(torch.autograd.grad(loss, x)[0].float(), acc=acc)

    def __call__(self, x, y):
        np.random.seed(self.random_seed)  # the reference's side effect on the global stream
        xd = torch.as_tensor(x).detach().to(self.device, torch.float32).contiguous()
        y = _targets(y, self.device)
        acc = torch.zeros((xd.shape[0],) + tuple(xd.shape[2:]), dtype=torch.float64, device=self.device)
        for s in range(self.n_samples):
            self.compute_gradients(self.noisy(xd, s), y, acc=acc)
        return (acc / self.n_samples).cpu().numpy()


class Saliency:
    """captum.attr.Saliency as the reference uses it: ``attribute(x, target=)`` -> |d out[i, target[i]]
    / dx| as a [N, C, H, W] tensor (captum's default ``abs=True``). ``maps`` is the reference's float32
    channel mean of it, [N, H, W] on the device."""

    def __init__(self, model):
        self.model = model
        self.device = _device_of(model)

    def _grads(self, x, target):
        xd = torch.as_tensor(x).detach().to(self.device, torch.float32).contiguous()
        return _input_grads(self.model, xd, _targets(target, self.device))

    def attribute(self, x, target=None, abs=True):
        g = self._grads(x, target)
        return g.abs() if abs else g

    def maps(self, x, target):
        return channel_mean(self._grads(x, target), absolute=True)


class IntegratedGradients:
    """captum.attr.IntegratedGradients as the reference uses it: zero baseline, per-sample
    out[i, target[i]], ``riemann_trapezoid`` (alphas linspace(0, 1, n_steps), step sizes 1 / (n - 1)
    with the two ends halved). ``attribute`` -> x * sum_k step_k * grad_k as a [N, C, H, W] tensor; the
    step sum is wam_trapz_f32's weighted form in float32. ``internal_batch_size`` bounds the rows of
    one forward (whole steps: at least one step of N rows), None takes all steps at once."""

    def __init__(self, model):
        self.model = model
        self.device = _device_of(model)

    def _avg_grads(self, xd, target, n_steps, internal_batch_size):
        if n_steps < 2:
            raise ValueError("riemann_trapezoid needs n_steps >= 2")
        N = xd.shape[0]
        alphas = np.linspace(0, 1, n_steps)
        steps = np.full(n_steps, 1.0 / (n_steps - 1))
        steps[0] /= 2
        steps[-1] /= 2
        weights = torch.as_tensor(steps.astype(np.float32)).to(self.device)
        per = n_steps if internal_batch_size is None else max(1, int(internal_batch_size) // N)
        acc = torch.zeros_like(xd)
        for k0 in range(0, n_steps, per):
            k1 = min(n_steps, k0 + per)
            xs = torch.cat([xd * float(a) for a in alphas[k0:k1]])
            g = _input_grads(self.model, xs, target.repeat(k1 - k0))
            _plan.trapz_stream(g, k1 - k0, 0, None, acc, weights=weights[k0:k1].contiguous())
        return acc

    def _prepare(self, x, target, method):
        if method != "riemann_trapezoid":
            raise ValueError("IntegratedGradients: only method='riemann_trapezoid' (the reference's) is provided, "
                             "got %r" % (method,))
        xd = torch.as_tensor(x).detach().to(self.device, torch.float32).contiguous()
        return xd, _targets(target, self.device)

    def attribute(self, x, target=None, method="riemann_trapezoid", n_steps=50, internal_batch_size=None,
                  return_convergence_delta=False):
        xd, t = self._prepare(x, target, method)
        attr = self._avg_grads(xd, t, n_steps, internal_batch_size) * xd
        if not return_convergence_delta:
            return attr
        with torch.no_grad():
            ends = self.model(torch.cat([xd, torch.zeros_like(xd)])).gather(1, t.repeat(2)[:, None])[:, 0]
        return attr, attr.flatten(1).sum(1) - (ends[:xd.shape[0]] - ends[xd.shape[0]:])

    def maps(self, x, target, method="riemann_trapezoid", n_steps=50, internal_batch_size=None):
        """The reference's float32 channel mean of ``attribute``, [N, H, W] on the device."""
        xd, t = self._prepare(x, target, method)
        return channel_mean(self._avg_grads(xd, t, n_steps, internal_batch_size), mult=xd)


# ------------------------------------------------------------------------------------ masked inputs
def _outputs(n, C, P, dev, want):
    """The (masked, u8, out) triple of the two mask entries with only ``want`` allocated."""
    masked = torch.empty((n, C, P), dtype=torch.float32, device=dev) if want == "masked" else None
    u8 = torch.empty((n, C, P), dtype=torch.uint8, device=dev) if want == "u8" else None
    out = torch.empty((n, C, P), dtype=torch.float32, device=dev) if want == "out" else None
    return masked, u8, out


def rank_mask_pixels(imgs, rank, n_iter, deletion, want="out"):
    """wam_rank_mask_pixels: imgs [sets, C, P] float32, rank [sets, P] int32 (device) -> the ``want``
    output ('masked', 'u8' or 'out') of all sets * (n_iter + 1) masked images, [sets * (n_iter + 1), C, P]."""
    sets, C, P = imgs.shape
    dev = imgs.device
    mean, std = norm_consts(C)
    masked, u8, out = _outputs(sets * (n_iter + 1), C, P, dev, want)
    ws = torch.empty(int(lib.wam_rank_mask_pixels_ws_bytes(sets, n_iter)) // 4, dtype=torch.float32, device=dev)
    check(lib.wam_rank_mask_pixels(sets, C, P, ptr(imgs.contiguous()), ptr(rank.contiguous()), n_iter, int(P / n_iter),
                                   int(bool(deletion)), mean, std, ptr(masked), ptr(u8), ptr(out), ptr(ws),
                                   stream_of(dev)))
    return {"masked": masked, "u8": u8, "out": out}[want]


def cell_mask_pixels(img, grid_masks, cell, want="out"):
    """wam_cell_mask_pixels: img [C, P] float32, grid_masks [n, grid_len] float32, cell [P] int32
    (device) -> the ``want`` output of the n masked images, [n, C, P]."""
    C, P = img.shape
    n, grid_len = grid_masks.shape
    mean, std = norm_consts(C)
    masked, u8, out = _outputs(n, C, P, img.device, want)
    check(lib.wam_cell_mask_pixels(C, P, ptr(img.contiguous()), n, grid_len, ptr(grid_masks.contiguous()), ptr(cell),
                                   mean, std, ptr(masked), ptr(u8), ptr(out), stream_of(img.device)))
    return {"masked": masked, "u8": u8, "out": out}[want]


class EvalImageBaselines:
    """src/evaluators.py:805-1180 -- insertion, deletion (Petsiuk et al.) and mu-fidelity (Bhatt et al.)
    of a pixel-domain attribution method, on the device. Same positional arguments, methods, return
    values and side attributes (``explanations`` computed once and cached -- a caller may assign it
    before the first call --, ``insertion_curves``, ``deletion_curves``).

    ``method_name``: 'gradcam', 'gradcampp' (``layers`` = the target module), 'saliency',
    'integratedgrad', 'smoothgrad'. 'guided_backprop', 'layercam', 'lrp' and 'srd' need packages this
    project does not carry and raise NotImplementedError naming the package; any other name is a
    ValueError here, at construction (the reference constructs and fails later with an AttributeError
    on ``self.method``).

    Kept from the reference: the ranking is of the signed explanation; n_comp = int(P / n_iter) and the
    last mask is forced full; images go through show(); Saliency and Integrated Gradients maps are the
    float32 channel mean of the attribution; mu-fidelity seeds numpy with ``random_seed``, draws its
    subsets with Python's global ``random``, its baseline-state masks as float32 uniforms, sums the
    importance without a Gaussian filter, keeps int(ceil(sample_size) / batch_size) (sic) batches of
    rows and averages spearmanr's (rho, p-value) pair. Ties: ``tie_order`` as in Eval2DWAM.

    Not kept: the model sees ``eval_batch`` rows per forward (several images' masks in one) where the
    reference runs ``batch_size`` = 2; ``batch_size`` still decides the row count of mu-fidelity as
    above; Integrated Gradients bounds its forwards by ``eval_batch`` rows as well.

    Transform: the default (Resize((224, 224)), ToTensor, Normalize(ImageNet)) runs on the device -- fused
    into the mask kernels at 224 x 224, Pillow-exact bilinear otherwise; a user ``transform`` is applied
    on the host to PIL images built from the kernels' uint8 output."""

    def __init__(self, method_name, model, layers=None, transform=None, random_seed=42, batch_size=2, *,
                 tie_order="stable", eval_batch=520):
        if method_name in _NEEDS:
            raise NotImplementedError("EvalImageBaselines: method %r needs %s, which this project does not carry"
                                      % (method_name, _NEEDS[method_name]))
        if method_name not in METHODS:
            raise ValueError("EvalImageBaselines: unknown method %r (one of %s)" % (method_name, ", ".join(METHODS)))
        self.transform = transform
        self.random_seed = random_seed
        self.method_name = method_name
        self.batch_size = batch_size
        self.model = model
        self.explanations = None
        self.device = self._dev = _device_of(model)
        self.tie_order = check_tie_order(tie_order)
        self.eval_batch = eval_batch
        self.insertion_curves = []
        self.deletion_curves = []
        if method_name == "gradcam":
            self.method = GradCAM(model, layers)
        elif method_name == "gradcampp":
            self.method = GradCAMPlusPlus(model, layers)
        elif method_name == "saliency":
            self.method = Saliency(model)
        elif method_name == "integratedgrad":
            self.method = IntegratedGradients(model)
        else:
            self.method = SmoothGrad(model)

    # -------------------------------------------------------------------- device pipeline
    def _model_inputs(self, produce, n, C, H, W):
        """produce(want) -> one output of a mask entry for n images; returns what the model reads."""
        if self.transform is not None:
            from PIL import Image
            u8 = np.moveaxis(produce("u8").cpu().numpy().reshape(n, C, H, W), 1, 3)
            ims = [Image.fromarray(a[:, :, 0] if C == 1 else a) for a in u8]
            return torch.stack([torch.as_tensor(np.asarray(self.transform(im))).float() for im in ims]).to(self._dev)
        if (H, W) == (224, 224):  # Resize((224, 224)) is the identity: the fused output
            return produce("out").view(n, C, H, W)
        mean, std = norm_consts(C)
        return resize_default(self._dev, produce("masked"), n, C, H, W, mean, std)[0]

    def _eval_rows(self, inputs, label, n_rows):
        """Class probabilities of the first n_rows inputs, eval_batch rows per forward."""
        out = [class_probs(self.model, inputs[s:min(n_rows, s + self.eval_batch)], label).astype(np.float32)
               for s in range(0, n_rows, self.eval_batch)]
        return np.concatenate(out) if out else np.empty(0, dtype=np.float32)

    def _cell_inputs(self, image, grid_masks, grid_size):
        C, H, W = image.shape
        n = grid_masks.shape[0]
        cell = cell_map(grid_size, (H, W), self._dev)
        g = torch.as_tensor(np.ascontiguousarray(grid_masks, dtype=np.float32)).to(self._dev).reshape(n, -1)
        img = image.reshape(C, H * W)
        return self._model_inputs(lambda want: cell_mask_pixels(img, g, cell, want), n, C, H, W)

    # -------------------------------------------------------------------- reference API
    def compute_explanations(self, x, y):
        """src/evaluators.py:904-959: numpy [N, H, W] (float64 for smoothgrad, float32 otherwise)."""
        if self.method_name in ("smoothgrad", "gradcam", "gradcampp"):
            return self.method(x, y)
        if self.method_name == "integratedgrad":
            return self.method.maps(x, y, method="riemann_trapezoid", n_steps=50,
                                    internal_batch_size=self.eval_batch).cpu().numpy()
        return self.method.maps(x, y).cpu().numpy()

    def evaluate_auc(self, x, y, mode, n_iter=64):
        """src/evaluators.py:961-1016: AUC of the class probability along the insertion (deletion)
        path of the explanation's ranking."""
        n_samples = x.shape[0]
        images = show_images(x, self._dev)
        if self.explanations is None:
            self.explanations = self.compute_explanations(x, y)
        M = n_iter + 1
        C, H, W = images[0].shape
        scores, predicted_probs = [], []
        per_call = max(1, self.eval_batch // M)
        for s0 in range(0, n_samples, per_call):
            group = list(range(s0, min(n_samples, s0 + per_call)))
            imgs = torch.stack([images[s] for s in group]).reshape(len(group), C, H * W)
            rank = descending_ranks(np.stack([np.asarray(self.explanations[s]).reshape(-1) for s in group]),
                                    self._dev, self.tie_order)
            inputs = self._model_inputs(lambda want: rank_mask_pixels(imgs, rank, n_iter, mode == "deletion", want),
                                        len(group) * M, C, H, W)
            with torch.no_grad():
                preds = self.model(inputs).float().cpu().numpy()
            for p in class_curves(preds, M, [y[s] for s in group]):
                p = p.tolist()
                scores.append(compute_auc(np.array(p)))  # float64, where the WAM evaluators stay in float32
                predicted_probs.append(p)
        return scores, predicted_probs

    def insertion(self, x, y, n_iter=128):
        scores, predicted_probs = self.evaluate_auc(x, y, "insertion", n_iter=n_iter)
        self.insertion_curves = predicted_probs
        return scores

    def deletion(self, x, y, n_iter=128):
        scores, predicted_probs = self.evaluate_auc(x, y, "deletion", n_iter=n_iter)
        self.deletion_curves = predicted_probs
        return scores

    def compute_baseline_state(self, image, label, grid_size, batch_size, sample_size):
        """src/evaluators.py:1036-1072: the float32 uniform random superpixel mask whose masked image
        has the lowest class probability. ``image``: [C, H, W] on the device (show_images)."""
        source_masks = np.random.uniform(size=(sample_size, grid_size, grid_size)).astype(np.float32)
        ys = self._eval_rows(self._cell_inputs(image, source_masks, grid_size), label, sample_size)
        return source_masks[int(np.argmin(ys)), :, :]

    def mu_fidelity(self, x, y, grid_size=28, sample_size=512, subset_size=157):
        """src/evaluators.py:1074-1180."""
        if self.explanations is None:
            self.explanations = self.compute_explanations(x, y)
        np.random.seed(self.random_seed)
        dev = self._dev
        xd = torch.as_tensor(x).detach().to(dev, torch.float32)
        with torch.no_grad():
            base = softmax(self.model(xd).float().cpu().numpy())
        base_probs = [base[i, y[i]] for i in range(len(y))]
        images = show_images(x, dev)
        H, W = xd.shape[2], xd.shape[3]
        cell = cell_map(grid_size, (H, W), dev)
        n_rows = min(sample_size, int(np.ceil(sample_size) / self.batch_size) * self.batch_size)
        mu = []
        for i in range(len(self.explanations)):
            indices = generate_subsets(grid_size, subset_size, sample_size)
            bmask = self.compute_baseline_state(images[i], y[i], grid_size, self.batch_size, sample_size)
            masks = np.ones((sample_size, grid_size, grid_size), dtype=np.float32)
            sub = np.zeros((sample_size, grid_size, grid_size), dtype=np.float32)
            for j, index_set in enumerate(indices):
                cx, cy = zip(*index_set)
                masks[j, cx, cy] = bmask[cx, cy]
                sub[j, cx, cy] = 1
            altered = self._eval_rows(self._cell_inputs(images[i], masks, grid_size), y[i], n_rows)
            preds = base_probs[i] - altered
            expl = torch.as_tensor(np.ascontiguousarray(self.explanations[i]), dtype=torch.float64).to(dev)
            mu.append(np.nanmean(spearmanr(preds, masked_sums(expl, sub, cell))))
        return mu
