"""Python side of the C-ABI: plans (cached per device) and thin typed wrappers of every entry
point of include/wam_hip.h. torch allocates every device buffer; every call is asynchronous on
torch's current stream of the tensor's device."""
import collections
import ctypes
import threading

import numpy as np
import torch

from . import filters
from ._lib import c_f32, c_i64, c_vp, check, lib, ptr, require_cuda, stream_of

_CACHE = {}
_LOCK = threading.Lock()
PLAN_GENERIC = 1

class Plan:
    """Immutable transform plan (ndim, spatial shape, levels, wavelet, mode) on one device."""

    def __init__(self, ndim, shape, levels, wavelet, mode, device, flags=0):
        self.ndim = int(ndim)
        self.shape = tuple(int(s) for s in shape)
        self.levels = int(levels)
        self.wavelet = filters.get_wavelet(wavelet)
        self.mode = mode
        self.device = torch.device(device)
        self.flags = flags
        L = len(self.wavelet.dec_lo)
        arr = lambda v: (ctypes.c_double * L)(*v)
        shp = (ctypes.c_int64 * self.ndim)(*self.shape)
        handle = c_vp()
        with torch.cuda.device(self.device):
            check(lib.wam_plan_create_ex(ctypes.byref(handle), self.ndim, shp, self.levels, arr(self.wavelet.dec_lo),
                                         arr(self.wavelet.dec_hi), arr(self.wavelet.rec_lo),
                                         arr(self.wavelet.rec_hi), L, filters.mode_id(mode), flags))
        self._h = handle
        self.L = L
        self.nbands = lib.wam_plan_num_bands(handle)
        dims = (ctypes.c_int64 * self.ndim)()
        self.band_shapes = []
        for b in range(self.nbands):
            check(lib.wam_plan_band_shape(handle, b, dims))
            self.band_shapes.append(tuple(dims[:]))
        self.band_offsets = [lib.wam_plan_band_offset(handle, b) for b in range(self.nbands + 1)]
        self.coeff_numel = lib.wam_plan_coeff_numel(handle)
        check(lib.wam_plan_rec_shape(handle, dims))
        self.rec_shape = tuple(dims[:])
        self._ws = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and lib is not None:
            lib.wam_plan_destroy(h)
            self._h = None

    # ---------------------------------------------------------------- layout helpers
    @property
    def handle(self):
        return self._h

    def workspace(self, batch):
        n = int(lib.wam_plan_workspace_bytes(self._h, batch))
        ws = self._ws.get("buf")
        if ws is None or ws.numel() < n:
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._ws["buf"] = ws
        return ws

    def split(self, flat, batch, lead=None):
        """Band views of a band-major coefficient buffer; each band reshaped to lead + band dims."""
        lead = (batch,) if lead is None else tuple(lead)
        out = []
        for b in range(self.nbands):
            n = int(np.prod(self.band_shapes[b]))
            o = batch * self.band_offsets[b]
            out.append(flat[o:o + batch * n].view(lead + self.band_shapes[b]))
        return out

    def band_level(self, b):
        """(level index 0 = finest, sub index) of band b; approximation -> (levels-1, -1)."""
        if b == 0:
            return self.levels - 1, -1
        per = (1 << self.ndim) - 1
        return self.levels - 1 - (b - 1) // per, (b - 1) % per

    # ---------------------------------------------------------------- transforms
    def wavedec(self, x, out=None):
        """x: [batch, *shape] fp32 cuda -> band-major flat coefficients [batch * coeff_numel]."""
        require_cuda(x, "x")
        x = x.contiguous()
        batch = x.numel() // int(np.prod(self.shape))
        if tuple(x.shape[-self.ndim:]) != self.shape:
            raise ValueError("input spatial shape %s does not match the plan %s" % (tuple(x.shape), self.shape))
        if out is None:
            out = torch.empty(batch * self.coeff_numel, dtype=torch.float32, device=x.device)
        ws = self.workspace(batch)
        check(lib.wam_wavedec(self._h, batch, ptr(x), ptr(out), ptr(ws), stream_of(x.device)))
        return out

    def waverec(self, flat, batch, alphas=None, out=None):
        """flat band-major coefficients -> [n_alpha, batch, *rec_shape] (n_alpha = 1 without alphas)."""
        require_cuda(flat, "coefficients")
        n_alpha = 1 if alphas is None else len(alphas)
        a = None if alphas is None else (c_f32 * n_alpha)(*[float(np.float32(v)) for v in alphas])
        if out is None:
            out = torch.empty((n_alpha, batch) + self.rec_shape, dtype=torch.float32, device=flat.device)
        ws = self.workspace(batch)
        check(lib.wam_waverec(self._h, batch, ptr(flat.contiguous()), a, n_alpha, ptr(out), ptr(ws),
                              stream_of(flat.device)))
        return out

    # ---- ranked synthesis (evaluate_ranked.hip): one helper behind the 3D, 2D and 1D entries
    def _ranked_route(self, sym):
        r = getattr(lib, sym + "_route")(self._h)
        if r < 0:
            check(-r)
        return r

    def _waverec_ranked(self, sym, key, dims, flat, rank, pos, n_iter, n_comp, deletion, route, out, lead=None,
                        want_max=None):
        """lib.<sym> and its workspace query. dims: the entry's leading counts, (sets,) or (images, channels);
        rank holds dims[0] rows. key: the workspace's slot in the plan's cache. lead: the leading dims of a
        new `out`, (items * (n_iter + 1),) unless given. want_max None: the entry takes no row_max.
        Returns (out, row_max)."""
        require_cuda(flat, "coefficients")
        flat, rank, pos = flat.contiguous(), rank.contiguous(), pos.contiguous()
        if rank.dtype != torch.int32 or pos.dtype != torch.int32:
            raise TypeError("wam_amd: rank and pos must be int32")
        items = int(np.prod(dims))
        if (flat.numel() != items * self.coeff_numel or pos.numel() != self.coeff_numel or rank.dim() != 2
                or rank.shape[0] != dims[0]):
            raise ValueError("expected %s x %d coefficients, %d positions and %d rank rows"
                             % (" x ".join(map(str, dims)), self.coeff_numel, self.coeff_numel, dims[0]))
        M = int(n_iter) + 1
        if out is None:
            out = torch.empty((lead or (items * M,)) + self.rec_shape, dtype=torch.float32, device=flat.device)
        row_max = torch.empty(items * M, dtype=torch.float32, device=flat.device) if want_max else None
        ws = None
        # 3D: the plan's own route keeps a workspace at hand only when it is route 0
        n = int(getattr(lib, sym + "_workspace_bytes")(self._h, *dims, n_iter, route))
        if n:
            ws = self._ws.get(key)
            if ws is None or ws.numel() < n:
                ws = self._ws[key] = torch.empty(n, dtype=torch.uint8, device=self.device)
        extra = () if want_max is None else (ptr(row_max),)
        check(getattr(lib, sym)(self._h, *dims, ptr(flat), ptr(rank), rank.shape[1], ptr(pos), n_iter, n_comp,
                                int(bool(deletion)), route, ptr(out), *extra, ptr(ws), stream_of(flat.device)))
        return out, row_max

    @property
    def ranked_route(self):
        """The route waverec_ranked takes by itself (wam_waverec_ranked_route): 0 = mask expansion +
        waverec, 1 = the fused 3D Haar kernel. 3D plans only."""
        return self._ranked_route("wam_waverec_ranked")

    def waverec_ranked(self, flat, sets, rank, pos, n_iter, n_comp, deletion, route=-1, out=None):
        """The n_iter + 1 masked reconstructions of each of `sets` volumes (wam_waverec_ranked): flat
        band-major coefficients of the sets, rank int32 [sets, rank_len] and pos int32 [coeff_numel] as
        for wam_rank_mask_coeffs -> [sets * (n_iter + 1), *rec_shape], volume s * (n_iter + 1) + m.
        route: -1 the plan's own, 0 expansion + waverec (workspace from the plan), 1 the fused kernel."""
        return self._waverec_ranked("wam_waverec_ranked", "ranked", (sets,), flat, rank, pos, n_iter, n_comp,
                                    deletion, route, out)[0]

    # ---- cell-mask synthesis (evaluate_cells.hip)
    @property
    def cells_route(self):
        """The route waverec_cells takes by itself (wam_waverec_cells_route): 0 = mask expansion +
        waverec, 1 = the fused 3D Haar kernel. 3D plans only."""
        return self._ranked_route("wam_waverec_cells")

    def waverec_cells(self, flat, sets, slot, grid, route=-1, out=None):
        """The reconstructions of each of `sets` volumes under its own n_masks float masks
        (wam_waverec_cells): flat band-major coefficients of the sets, slot int32 [coeff_numel] (the grid
        cell of every coefficient; outside [0, grid_len): the coefficient is left as it is) and grid
        float32 [sets, n_masks, grid_len] -> [sets * n_masks, *rec_shape], volume s * n_masks + m.
        route: -1 the plan's own, 0 expansion + waverec (workspace from the plan), 1 the fused kernel."""
        require_cuda(flat, "coefficients")
        require_cuda(grid, "grid")
        flat, slot, grid = flat.contiguous(), slot.contiguous(), grid.contiguous()
        if slot.dtype != torch.int32:
            raise TypeError("wam_amd: slot must be int32")
        if (flat.numel() != sets * self.coeff_numel or slot.numel() != self.coeff_numel or grid.dim() != 3
                or grid.shape[0] != sets):
            raise ValueError("expected %d x %d coefficients, %d slots and %d sets of masks"
                             % (sets, self.coeff_numel, self.coeff_numel, sets))
        n_masks, grid_len = int(grid.shape[1]), int(grid.shape[2])
        if out is None:
            out = torch.empty((sets * n_masks,) + self.rec_shape, dtype=torch.float32, device=flat.device)
        # the plan's own route falls back to route 0 above the fused kernel's largest grid: size for it
        sized = 0 if route < 0 and grid_len > CELLS_FUSED_MAX_GRID else route
        ws = None
        n = int(lib.wam_waverec_cells_workspace_bytes(self._h, sets, n_masks, sized))
        if n:
            ws = self._ws.get("cells")
            if ws is None or ws.numel() < n:
                ws = self._ws["cells"] = torch.empty(n, dtype=torch.uint8, device=self.device)
        check(lib.wam_waverec_cells(self._h, sets, ptr(flat), ptr(slot), n_masks, grid_len, ptr(grid), route, ptr(out),
                                    ptr(ws), stream_of(flat.device)))
        return out

    def ranked2_route(self):
        """The route waverec2_ranked takes by itself (wam_waverec2_ranked_route): 0 = mask expansion +
        waverec, 1 = the fused plane-resident kernel. 2D plans only."""
        return self._ranked_route("wam_waverec2_ranked")

    def waverec2_ranked(self, flat, images, channels, rank, pos, n_iter, n_comp, deletion, route=-1, out=None):
        """The n_iter + 1 masked reconstructions of each of `images` images of `channels` planes
        (wam_waverec2_ranked): flat band-major coefficients of the images * channels planes, rank int32
        [images, rank_len] and pos int32 [coeff_numel] -> [images, n_iter + 1, channels, *rec_shape].
        route: -1 the plan's own, 0 expansion + waverec, 1 the fused kernel; the workspace of either comes
        from the plan."""
        return self._waverec_ranked("wam_waverec2_ranked", "ranked2", (images, channels), flat, rank, pos, n_iter,
                                    n_comp, deletion, route, out, lead=(images, int(n_iter) + 1, channels))[0]

    def ranked1_route(self):
        """The route waverec1_ranked takes by itself (wam_waverec1_ranked_route): 0 = mask expansion +
        waverec, 1 = the fused tile kernel. 1D plans only."""
        return self._ranked_route("wam_waverec1_ranked")

    def waverec1_ranked(self, flat, sets, rank, pos, n_iter, n_comp, deletion, route=-1, out=None, want_max=True):
        """The n_iter + 1 masked reconstructions of each of `sets` signals and their signed maxima
        (wam_waverec1_ranked): flat band-major coefficients of the sets, rank int32 [sets, rank_len] and
        pos int32 [coeff_numel] as for wam_rank_mask_coeffs -> (out [sets * (n_iter + 1), rec_len],
        row_max [sets * (n_iter + 1)] or None without want_max). route: -1 the plan's own, 0 expansion +
        waverec, 1 the fused kernel; the workspace of either comes from the plan."""
        return self._waverec_ranked("wam_waverec1_ranked", "ranked1", (sets,), flat, rank, pos, n_iter, n_comp,
                                    deletion, route, out, want_max=bool(want_max))

    def waverec_bf16_nhwc(self, flat, batch, channels, alphas=None, out=None):
        """flat band-major coefficients of `batch` planes (images x channels) -> the reconstruction as
        bf16 images [n_alpha * batch / channels, channels, *rec_shape] in channels_last memory (the
        explained model's input dtype and layout; RNE rounding, as torch's cast). WAM_CAP_BF16_NHWC."""
        require_cuda(flat, "coefficients")
        n_alpha = 1 if alphas is None else len(alphas)
        a = None if alphas is None else (c_f32 * n_alpha)(*[float(np.float32(v)) for v in alphas])
        if out is None:
            out = torch.empty((n_alpha * batch // channels, channels) + self.rec_shape, dtype=torch.bfloat16,
                              device=flat.device, memory_format=torch.channels_last)
        check(lib.wam_waverec_bf16_nhwc(self._h, batch, ptr(flat.contiguous()), a, n_alpha, channels, ptr(out),
                                        stream_of(flat.device)))
        return out

    def adjoint(self, grad, out=None):
        """grad [batch, *rec_shape] -> band-major coefficient gradients (waverec's VJP)."""
        require_cuda(grad, "grad")
        grad = grad.contiguous()
        batch = grad.numel() // int(np.prod(self.rec_shape))
        if out is None:
            out = torch.empty(batch * self.coeff_numel, dtype=torch.float32, device=grad.device)
        ws = self.workspace(batch)
        check(lib.wam_waverec_adjoint(self._h, batch, ptr(grad), ptr(out), ptr(ws), stream_of(grad.device)))
        return out

    def wavedec_adjoint(self, coeff_grads_flat, batch, out=None):
        """band-major coefficient gradients -> grad_x [batch, *shape] (wavedec's VJP)."""
        require_cuda(coeff_grads_flat, "coefficient gradients")
        flat = coeff_grads_flat.contiguous()
        if flat.numel() != batch * self.coeff_numel:
            raise ValueError("expected %d x %d coefficient gradients, got %d" % (batch, self.coeff_numel,
                                                                                   flat.numel()))
        if out is None:
            out = torch.empty((batch,) + self.shape, dtype=torch.float32, device=flat.device)
        ws = self.workspace(batch)  # never smaller than wam_wavedec_adjoint_workspace_bytes
        check(lib.wam_wavedec_adjoint(self._h, batch, ptr(flat), ptr(out), ptr(ws), stream_of(flat.device)))
        return out

    @property
    def wavedec_adjoint_routes(self):
        """Per level, finest first: 'axis' or 'fold2d' (wam_plan_wavedec_adjoint_route)."""
        return [("axis", "fold2d")[lib.wam_plan_wavedec_adjoint_route(self._h, l)] for l in range(self.levels)]

    # ---------------------------------------------------------------- fused WAM passes
    @property
    def caps(self):
        return lib.wam_plan_caps(self._h)

    @property
    def routes(self):
        """The kernel family serving each transform of this plan (wam_plan_describe), e.g.
        'ana=plane|rows,rows,rows adj=plane|rows,rows,rows syn=plane|colstrip maps=plane caps=7'."""
        buf = ctypes.create_string_buffer(512)
        check(lib.wam_plan_describe(self._h, buf, len(buf)))
        return buf.value.decode()

    def wavedec_noisy(self, x, sigma, n_samples, images, channels, seed, sample_base=0, out=None, image_base=0):
        """coefficients of x + sigma_i N(0,1) (Philox) for n_samples x images x channels planes;
        image_base = global index of x's first image (Philox counter of a batch-sharded rank)."""
        require_cuda(x, "x")
        x = x.contiguous()
        batch = n_samples * images * channels
        if out is None:
            out = torch.empty(batch * self.coeff_numel, dtype=torch.float32, device=x.device)
        ws = self.workspace(batch)
        check(lib.wam_wavedec_noisy_ex(self._h, n_samples, images, channels, ptr(x), ptr(sigma),
                                       ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), sample_base, image_base, ptr(out),
                                       ptr(ws), stream_of(x.device)))
        return out

    def adjoint_maps(self, grad, groups, group_items, channels, full=False, maps=None, band_max=None):
        """waverec VJP fused with the channel-mean |.| epilogue -> (maps, band_max[, coeff grads]).
        grad: fp32 [images * channels, *rec_shape], or a bf16 channels_last [images, channels,
        *rec_shape] tensor (the model's own gradient; WAM_CAP_BF16_NHWC, full=False). maps / band_max:
        optional outputs (band_max zero-filled by the caller)."""
        if grad.dtype == torch.bfloat16:
            require_cuda(grad[:0].float(), "grad")  # the device check only
        else:
            require_cuda(grad, "grad")
        images = groups * group_items
        dev = grad.device
        maps = torch.empty(images * self.coeff_numel, dtype=torch.float32, device=dev) if maps is None else maps
        bmax = torch.zeros((groups, self.nbands), dtype=torch.float32, device=dev) if band_max is None else band_max
        if grad.dtype == torch.bfloat16:
            if full or grad.dim() != 4:
                raise ValueError("bf16 input gradients: an [images, channels, H, W] tensor, full=False")
            nhwc = grad.is_contiguous(memory_format=torch.channels_last)
            if not (nhwc or grad.is_contiguous()):
                grad = grad.contiguous(memory_format=torch.channels_last)
                nhwc = True
            check(lib.wam_waverec_adjoint_maps_bf16(self._h, groups, group_items, channels, int(nhwc), ptr(grad),
                                                    ptr(maps), ptr(bmax), stream_of(dev)))
            return maps, bmax, None
        grad = grad.contiguous()
        cg = torch.empty(images * channels * self.coeff_numel, dtype=torch.float32, device=dev) if full else None
        ws = self.workspace(images * channels)
        check(lib.wam_waverec_adjoint_maps(self._h, groups, group_items, channels, ptr(grad), ptr(maps), ptr(bmax),
                                           ptr(cg), ptr(ws), stream_of(dev)))
        return maps, bmax, cg


def get_plan(ndim, shape, levels, wavelet, mode, device, generic=False, flags=None):
    w = filters.get_wavelet(wavelet)
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    fl = (PLAN_GENERIC if generic else 0) if flags is None else int(flags)
    key = (ndim, tuple(int(s) for s in shape), int(levels), w, mode, device, fl)
    with _LOCK:
        p = _CACHE.get(key)
        if p is None:
            p = Plan(ndim, shape, levels, w, mode, device, fl)
            _CACHE[key] = p
    return p


PLAN_NO_ROWS = 2
PLAN_NO_PLANE = 4
PLAN_NO_COOP = 8
PLAN_FORCE_COOP = 16
CAP_NOISY_WAVEDEC = 1
CAP_ADJOINT_MAPS = 2
CAP_BF16_NHWC = 4
CELLS_FUSED_MAX_GRID = 65535  # the largest grid_len route 1 of wam_waverec_cells takes (include/wam_hip.h)


def timing_enable(on=True):
    lib.wam_timing_enable(1 if on else 0)


def timing_drain():
    """[(kernel name, ms, algorithmic bytes)] for every launch since the last drain."""
    out = []
    cap = 4096
    while True:
        names = ctypes.create_string_buffer(64 * cap)
        ms = (c_f32 * cap)()
        nb = (ctypes.c_double * cap)()
        n = lib.wam_timing_drain(cap, names, ms, nb)
        for i in range(n):
            out.append((names.raw[64 * i:64 * (i + 1)].split(b"\0", 1)[0].decode(), ms[i], nb[i]))
        if n < cap:
            return out


# -------------------------------------------------------------------- WAM epilogue wrappers
# (device, stream, items, len) -> zero-initialised workspace of the split sigma reduction (its
# arrival counters are reset by every call, so one buffer serves the calls of that shape issued in
# order on one stream; calls on another stream get their own); least recently used entries go first
_SIGMA_WS = collections.OrderedDict()
_SIGMA_WS_MAX = 16


def item_sigma(x, item_stride, length, spread):
    """sigma_i = fp32(spread) * (max - min) of item i (lib/wam_2D.py:396-399, lib/wam_1D.py:311-314,
    lib/wam_3D.py:567-569), as a full-chip split reduction."""
    items = x.numel() // item_stride
    sigma = torch.empty(items, dtype=torch.float32, device=x.device)
    if items == 0:
        return sigma
    st = stream_of(x.device)
    key = (str(x.device), int(st.value or 0), int(items), int(length))
    ws = _SIGMA_WS.get(key)
    if ws is None:
        nb = int(lib.wam_item_sigma_ws_bytes(items, length))
        ws = _SIGMA_WS[key] = torch.zeros((nb + 7) // 8, dtype=torch.float64, device=x.device)
        while len(_SIGMA_WS) > _SIGMA_WS_MAX:
            _SIGMA_WS.popitem(last=False)
    _SIGMA_WS.move_to_end(key)
    check(lib.wam_item_sigma_ws(items, item_stride, length, ptr(x), float(np.float32(spread)), ptr(sigma), ptr(ws),
                                ws.numel() * 8, st))
    return sigma


def noise_add(x, sigma, n_samples, items, item_stride, noised_len, seed=0, sample_base=0, host_noise=None, out=None,
              item_base=0):
    if out is None:
        out = torch.empty((n_samples * items * item_stride,), dtype=torch.float32, device=x.device)
    check(lib.wam_noise_add_ex(n_samples, items, item_stride, noised_len, ptr(x), ptr(sigma), ptr(host_noise),
                               ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), sample_base, item_base, ptr(out),
                               stream_of(x.device)))
    return out


def peak_divide(x, row_max, zero_silent=False, out=None):
    """x [rows, len] float32 / row_max [rows] (wam_peak_divide; in place without `out`) -> (out, silent
    int32 [rows]: row_max == 0). zero_silent: a silent row is left as it is."""
    require_cuda(x, "x")
    rows, length = x.shape
    if not x.is_contiguous() or row_max.numel() != rows or row_max.dtype != torch.float32:
        raise ValueError("peak_divide: contiguous [rows, len] rows and %d float32 maxima" % rows)
    out = x if out is None else out
    silent = torch.empty(rows, dtype=torch.int32, device=x.device)
    check(lib.wam_peak_divide(rows, length, ptr(x), ptr(row_max), ptr(out), ptr(silent), int(bool(zero_silent)),
                              stream_of(x.device)))
    return out, silent


def subband_maps(plan, coeff_grads, groups, group_items, channels, maps=None, band_max=None, want_max=True):
    """|channel mean| maps (item-major) and per-group band maxima (None when want_max=False)."""
    items = groups * group_items
    dev = coeff_grads.device
    if maps is None:
        maps = torch.empty(items * plan.coeff_numel, dtype=torch.float32, device=dev)
    if not want_max:
        band_max = None
    elif band_max is None:
        band_max = torch.zeros((groups, plan.nbands), dtype=torch.float32, device=dev)
    else:
        band_max.zero_()
    check(lib.wam_subband_maps(plan.handle, groups, group_items, channels, ptr(coeff_grads), ptr(maps),
                               ptr(band_max), stream_of(dev)))
    return maps, band_max


_INV = {}


def _inverse_map(gmap, maps_item_len):
    """(dst, cband) per packed coefficient from the per-pixel (src, band) mosaic map, or None when
    the map is not injective (cached per map)."""
    src, band = gmap
    key = (src.data_ptr(), band.data_ptr(), int(maps_item_len))
    if key not in _INV:
        valid = src >= 0
        pix = torch.nonzero(valid).reshape(-1)
        s = src[valid].long()
        dst = torch.full((maps_item_len,), -1, dtype=torch.int32, device=src.device)
        cband = torch.zeros((maps_item_len,), dtype=torch.int32, device=src.device)
        ok = s.numel() == 0 or (int(s.max()) < maps_item_len and torch.unique(s).numel() == s.numel())
        if ok:
            dst[s] = pix.to(torch.int32)
            cband[s] = band[valid]
        _INV[key] = (dst, cband, gmap) if ok else None  # gmap kept alive: its pointers are the key
    v = _INV[key]
    return None if v is None else v[:2]


def frame_accumulate(groups, group_items, gmap, maps, maps_item_len, band_max, n_bands, normalize, frame):
    src, band = gmap
    inv = _inverse_map(gmap, maps_item_len)
    if inv is not None:  # coefficient order: contiguous map reads
        check(lib.wam_frame_accumulate_coef(groups, group_items, maps_item_len, src.numel(), ptr(inv[0]), ptr(inv[1]),
                                            ptr(maps), ptr(band_max), n_bands, int(bool(normalize)), ptr(frame),
                                            stream_of(frame.device)))
        return
    check(lib.wam_frame_accumulate(groups, group_items, src.numel(), ptr(src), ptr(band), ptr(maps),
                                   maps_item_len, ptr(band_max), n_bands, int(bool(normalize)), ptr(frame),
                                   stream_of(frame.device)))


def frame_trapz(groups, k0, group_items, gmap, maps, maps_item_len, band_max, n_bands, normalize, prev, acc,
                weights=None):
    src, band = gmap
    inv = _inverse_map(gmap, maps_item_len)
    if inv is not None:  # coefficient order: contiguous map reads (prev / acc are zero outside the mosaic)
        check(lib.wam_frame_trapz_coef(groups, k0, group_items, maps_item_len, src.numel(), ptr(inv[0]),
                                       ptr(inv[1]), ptr(maps), ptr(band_max), n_bands, int(bool(normalize)),
                                       ptr(weights), ptr(prev), ptr(acc), stream_of(acc.device)))
        return
    check(lib.wam_frame_trapz(groups, k0, group_items, src.numel(), ptr(src), ptr(band), ptr(maps), maps_item_len,
                              ptr(band_max), n_bands, int(bool(normalize)), ptr(weights), ptr(prev), ptr(acc),
                              stream_of(acc.device)))


def cube_accumulate(groups, k0, group_items, src, maps, maps_item_len, mode, n_total, acc, prev=None, weights=None):
    check(lib.wam_cube_accumulate(groups, k0, group_items, src.numel(), ptr(src), ptr(maps), maps_item_len, mode,
                                  float(n_total), ptr(weights), ptr(prev), ptr(acc), stream_of(acc.device)))


def accumulate_f32(src, groups, acc, scale=0.0):
    check(lib.wam_accumulate_f32(groups, acc.numel(), ptr(src), float(scale), ptr(acc), stream_of(acc.device)))


def trapz_stream(src, groups, k0, prev, acc, weights=None):
    if acc.dtype == torch.float64:
        check(lib.wam_trapz_f32(groups, k0, acc.numel(), ptr(src), ptr(weights), None, None, ptr(prev), ptr(acc),
                                stream_of(acc.device)))
    else:
        check(lib.wam_trapz_f32(groups, k0, acc.numel(), ptr(src), ptr(weights), ptr(prev), ptr(acc), None, None,
                                stream_of(acc.device)))


# second moments of the SmoothGrad samples: S (sum) and Q (sum of squares), float64, zeroed by the caller
def frame_moments(groups, group_items, gmap, maps, maps_item_len, band_max, n_bands, normalize, sum_, sumsq):
    """frame_accumulate's sum and the sum of squares of the same values, one pass over the maps."""
    src, band = gmap
    inv = _inverse_map(gmap, maps_item_len)
    if inv is not None:  # coefficient order: contiguous map reads
        check(lib.wam_frame_moments_coef(groups, group_items, maps_item_len, src.numel(), ptr(inv[0]), ptr(inv[1]),
                                         ptr(maps), ptr(band_max), n_bands, int(bool(normalize)), ptr(sum_),
                                         ptr(sumsq), stream_of(sum_.device)))
        return
    check(lib.wam_frame_moments(groups, group_items, src.numel(), ptr(src), ptr(band), ptr(maps), maps_item_len,
                                ptr(band_max), n_bands, int(bool(normalize)), ptr(sum_), ptr(sumsq),
                                stream_of(sum_.device)))


def cube_moments(groups, group_items, src, maps, maps_item_len, sum_, sumsq):
    check(lib.wam_cube_moments(groups, group_items, src.numel(), ptr(src), ptr(maps), maps_item_len, ptr(sum_),
                               ptr(sumsq), stream_of(sum_.device)))


def moments_f32(src, groups, sum_, sumsq):
    check(lib.wam_moments_f32(groups, sum_.numel(), ptr(src), ptr(sum_), ptr(sumsq), stream_of(sum_.device)))


MOMENT_KINDS = {"mean": 0, "smooth_sq": 1, "vargrad": 2}


def moments_finish(sum_, sumsq, n, kind, dtype=torch.float64):
    """(S, Q) over n samples -> S / n ('mean'), Q / n ('smooth_sq') or the population variance
    max(fma(-m, m, Q / n), 0), m = S / n ('vargrad'), as a float64 or float32 tensor of S's shape."""
    sum_, sumsq = sum_.contiguous(), sumsq.contiguous()
    out = torch.empty(sum_.shape, dtype=dtype, device=sum_.device)
    o64, o32 = (out, None) if dtype == torch.float64 else (None, out)
    check(lib.wam_moments_finish(sum_.numel(), ptr(sum_), ptr(sumsq), int(n), MOMENT_KINDS[kind], ptr(o64), ptr(o32),
                                 stream_of(sum_.device)))
    return out


def gaussian_filter3d(x, weights, radius):
    """scipy.ndimage.gaussian_filter (mode 'reflect') of float64 volumes on the device
    (wam_gaussian_filter3d): x [items, d, h, w] or [d, h, w] float64, weights[0 .. radius] the symmetric
    1-D kernel on the host (evalcore.gaussian_weights) -> a new tensor of x's shape; x is left untouched."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float64 or x.dim() not in (3, 4):
        raise TypeError("wam_amd: gaussian_filter3d takes a float64 CUDA (HIP) tensor [items, d, h, w] or [d, h, w]")
    x = x.contiguous()
    d, h, w = (int(v) for v in x.shape[-3:])
    wts = np.ascontiguousarray(weights, dtype=np.float64)
    if wts.size < radius + 1:
        raise ValueError("gaussian_filter3d: %d weights for radius %d" % (wts.size, radius))
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    check(lib.wam_gaussian_filter3d(x.numel() // (d * h * w), d, h, w, wts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    int(radius), ptr(x), ptr(tmp), ptr(out), stream_of(x.device)))
    return out


def reproject_scales(avg, levels, approx):
    """avg: [items, size, size] float64 cuda -> [items, levels(+1), size, size] float64."""
    items, size = avg.shape[0], avg.shape[1]
    out = torch.empty((items, levels + (1 if approx else 0), size, size), dtype=torch.float64, device=avg.device)
    check(lib.wam_reproject_scales(items, size, levels, int(bool(approx)), ptr(avg.contiguous()), ptr(out),
                                   stream_of(avg.device)))
    return out


def disentangle_scales(plan, maps, band_max, items, approx, size):
    """BaseWAM2D.disentangle_scales on device maps -> [items, J(+1), size, size] float64."""
    out = torch.empty((items, plan.levels + (1 if approx else 0), size, size), dtype=torch.float64,
                      device=maps.device)
    check(lib.wam_disentangle_scales(plan.handle, items, ptr(maps), ptr(band_max), int(bool(approx)), int(size),
                                     ptr(out), stream_of(maps.device)))
    return out
