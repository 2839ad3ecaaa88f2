"""Fused elementwise execution of a BN-folded ReLU network's input-gradient pass.

After ``model_opt`` folds BatchNorm into the convolutions, a ResNet input-gradient step is
convolutions (MIOpen, MFMA) plus per-channel bias adds, ReLUs, residual adds and ReLU masks.
Executed op by op in torch these elementwise steps are separate HBM passes over activation
tensors -- on MI355X about half of the c2 step (profiles/r01f_bench_kernel_stats.csv: torch
add / clamp / threshold_backward kernels next to the convolutions). ``fuse_elementwise``
rewrites the traced graph so each chain is one HIP kernel (wam_amd/csrc/model_ew.hip):

* ``conv -> relu``            -> ``ConvBiasReLU``: the convolution without bias, then
  y = max(y + b, 0) in place; backward = ReLU mask (one pass) + convolution backward-data.
* ``relu(a + s)`` where a / s are biased convolutions (bottleneck tail, downsample shortcut)
  -> the convolutions without bias and ``AddBiasReLU``: out = max((a + b_a) + (s + b_s), 0) in
  one pass; backward = one ReLU-mask pass whose result feeds both branches.
* where the tail's convolution is a pointwise one at a shape the in-tree GEMM serves (bf16, 64 ->
  256 and 128 -> 512 channels: csrc/model_pw.hip), the GEMM and the tail are ONE launch (the
  ``ConvNoBias`` defers to its ``AddBiasReLU``), and in a skip-linked identity block conv1's
  input-gradient GEMM carries the producer's ReLU mask and the parked skip gradient as its epilogue.
* the polyphase input convolution (``model_opt.InputConv2d``) followed by a ReLU gets the same
  bias + ReLU epilogue and a masked polyphase backward.
* in bf16 the ReLU producers also write one bit per element (out > 0) and the backward masks read
  that bit instead of the activation; where a fused tail's output feeds a downsample block, a
  ``GradFork`` hands it to both users so that the two gradients are summed under the producer's
  mask in one launch; the stem's max pool applies bias + ReLU to what it loads (``RELU_BITS``).

Only the pattern's own nodes are touched; everything else runs as traced. The functions are the
same as the graph's up to fp rounding (the bf16 tail sum rounds once instead of three times);
tests/test_model_opt.py compares outputs and input gradients with the unfused model on the GPU.
There is no CPU path for the fused ops: on a CPU model the rewrite is not applied.
"""
import operator
import os

import torch
import torch.fx as fx
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .model_opt import InputConv2d, _PolyphaseInputGrad  # noqa: F401

_DT = {torch.float32: 0, torch.bfloat16: 1}
_UNSUPPORTED = 3  # WAM_ERR_UNSUPPORTED: the operands are not ones the entry serves, nothing was written

# Packed ReLU masks, junction forks and the stem's fused bias + ReLU + pool. One
# switch for all three, read at every call: off (or WAM_MODEL_RELU_BITS=0) the model runs the
# activation-reading kernels and autograd's own gradient sums, with the same results bit for bit.
RELU_BITS = os.environ.get("WAM_MODEL_RELU_BITS", "1") != "0"


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("wam_amd fused model ops support float32 / bfloat16 activations, got %s" % t.dtype)


def _layout(t):
    """(tensor in a dense layout, inner) where the channel of flat element i is (i // inner) % C."""
    if t.dim() == 4 and t.shape[1] > 1 and t.shape[2] * t.shape[3] > 1:
        if t.is_contiguous(memory_format=torch.channels_last):
            return t, 1
        t = t.contiguous()
        return t, t.shape[2] * t.shape[3]
    t = t.contiguous()
    inner = 1
    for d in t.shape[2:]:
        inner *= d
    return t, inner


def _like(t, ref):
    """t in ref's memory layout (dense), so flat elementwise indexing lines up."""
    if ref.dim() == 4 and ref.is_contiguous(memory_format=torch.channels_last) and not ref.is_contiguous():
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


def _stream(t):
    return _lib.c_vp(torch.cuda.current_stream(t.device).cuda_stream)


def bias_act_(y, b, relu=True):
    y, inner = _layout(y)
    _lib.check(_lib.lib.wam_ew_bias_act(_dt(y), y.numel(), y.shape[1], inner, _lib.ptr(y),
                                        _lib.ptr(b.to(y.dtype).contiguous() if b is not None else None),
                                        int(relu), _stream(y)))
    return y


def add_bias_relu(a, ba, s, bs):
    a, inner = _layout(a)
    s = _like(s, a)
    out = torch.empty_like(a)
    cast = (lambda b: None if b is None else b.to(a.dtype).contiguous())
    _lib.check(_lib.lib.wam_ew_add_bias_relu(_dt(a), a.numel(), a.shape[1], inner, _lib.ptr(a), _lib.ptr(cast(ba)),
                                             _lib.ptr(s), _lib.ptr(cast(bs)), _lib.ptr(out), _stream(a)))
    return out


def relu_mask(g, y, g2=None):
    """y > 0 ? g (+ g2) : 0 in y's layout (made dense: the kernel indexes all operands flat)."""
    y = _like(y, y)
    g = _like(g, y)
    g2 = None if g2 is None else _like(g2, y)
    out = torch.empty_like(y)
    _lib.check(_lib.lib.wam_ew_relu_mask(_dt(y), y.numel(), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(y), _lib.ptr(out),
                                         _stream(y)))
    return out


def _is_cl(t):
    """The dense layout _like(., t) produces is channels_last (else plain contiguous)."""
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def _dense(t, cl):
    return t.contiguous(memory_format=torch.channels_last) if cl else t.contiguous()


def _bits_ok(t):
    return RELU_BITS and t.dtype == torch.bfloat16 and t.numel() > 0 and t.numel() % 8 == 0


def _new_bits(t):
    return torch.empty(t.numel() // 8, dtype=torch.uint8, device=t.device)


def bias_relu_bits_(y, b):
    """bias_act_(y, b, True) -> (y, packed mask of y > 0); the mask is None where the bits form does
    not serve the operands (or is switched off) and the plain kernel ran."""
    y, inner = _layout(y)
    if _bits_ok(y):
        bits = _new_bits(y)
        rc = _lib.lib.wam_ew_bias_act_bits(_dt(y), y.numel(), y.shape[1], inner, _lib.ptr(y),
                                           _lib.ptr(b.to(y.dtype).contiguous() if b is not None else None),
                                           _lib.ptr(bits), _stream(y))
        if rc == 0:
            return y, bits
        if rc != _UNSUPPORTED:
            _lib.check(rc)
    return bias_act_(y, b, True), None


def add_bias_relu_bits(a, ba, s, bs):
    """add_bias_relu(a, ba, s, bs) -> (out, packed mask of out > 0 or None, as bias_relu_bits_)."""
    if _bits_ok(a):
        a, inner = _layout(a)
        s = _like(s, a)
        out = torch.empty_like(a)
        bits = _new_bits(a)
        cast = (lambda b: None if b is None else b.to(a.dtype).contiguous())
        rc = _lib.lib.wam_ew_add_bias_relu_bits(_dt(a), a.numel(), a.shape[1], inner, _lib.ptr(a), _lib.ptr(cast(ba)),
                                                _lib.ptr(s), _lib.ptr(cast(bs)), _lib.ptr(out), _lib.ptr(bits),
                                                _stream(a))
        if rc == 0:
            return out, bits
        if rc != _UNSUPPORTED:
            _lib.check(rc)
    return add_bias_relu(a, ba, s, bs), None


def relu_mask_bits(g, bits, cl, g2=None):
    """bit ? g (+ g2) : 0 with the producer's packed mask; cl: the producer's output was channels_last
    (the mask is indexed flat in that layout, so g and g2 are made dense in it)."""
    g = _dense(g, cl)
    g2 = None if g2 is None else _dense(g2, cl)
    for retry in (False, True):
        if retry:  # a gradient view at an odd storage offset: fresh allocations are aligned
            g, g2 = g.clone(), (None if g2 is None else g2.clone())
        out = torch.empty_like(g)
        rc = _lib.lib.wam_ew_relu_mask_bits(_dt(g), g.numel(), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(bits),
                                            _lib.ptr(out), _stream(g))
        if rc != _UNSUPPORTED:
            break
    _lib.check(rc)
    return out


def _pool_ok(y, k, s, p):
    v = 8 if y.dtype == torch.bfloat16 else 4
    return (y.is_cuda and y.dim() == 4 and y.dtype in _DT and y.shape[1] % v == 0 and 2 * p <= k and k * k <= 127
            and y.is_contiguous(memory_format=torch.channels_last) and y.shape[0] <= 65535 and y.shape[2] <= 65535
            and y.shape[3] * (y.shape[1] // v) < 2 ** 30)


def maxpool_nhwc(y, k, s, p):
    """max_pool2d(y, k, s, p) of a channels_last activation -> (out, byte window index)."""
    n, c, h, w = y.shape
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    out = torch.empty((n, c, ho, wo), dtype=y.dtype, device=y.device, memory_format=torch.channels_last)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=y.device)
    _lib.check(_lib.lib.wam_ew_maxpool_nhwc(_dt(y), n, h, w, c, k, s, p, _lib.ptr(y), _lib.ptr(out), _lib.ptr(idx),
                                            _stream(y)))
    return out, idx


def bias_relu_maxpool_nhwc(x, b, k, s, p):
    """maxpool_nhwc(bias_act_(x, b, True), k, s, p) in one launch, x left as it is; None where the
    kernel does not serve the operands."""
    n, c, h, w = x.shape
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    out = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
    rc = _lib.lib.wam_ew_bias_maxpool_nhwc(_dt(x), n, h, w, c, k, s, p, _lib.ptr(x), _lib.ptr(b.to(x.dtype).contiguous()),
                                           _lib.ptr(out), _lib.ptr(idx), _stream(x))
    if rc == _UNSUPPORTED:
        return None
    _lib.check(rc)
    return out, idx


def maxpool_nhwc_backward(gy, idx, in_shape, k, s, p, relu):
    """Input gradient of maxpool_nhwc (channels_last); relu also applies the mask of the ReLU
    that produced the pooled input."""
    n, c, h, w = in_shape
    gy = gy.contiguous(memory_format=torch.channels_last)
    gx = torch.empty((n, c, h, w), dtype=gy.dtype, device=gy.device, memory_format=torch.channels_last)
    _lib.check(_lib.lib.wam_ew_maxpool_nhwc_backward(_dt(gy), n, h, w, c, k, s, p, _lib.ptr(gy), _lib.ptr(idx),
                                                     int(relu), _lib.ptr(gx), _stream(gy)))
    return gx


def _conv_nd(x, w, stride, padding, dilation, groups):
    return torch.ops.aten.convolution(x, w, None, stride, padding, dilation, False, [0] * len(stride), groups)


def _conv_grad_input(g, x, w, stride, padding, dilation, groups):
    return torch.ops.aten.convolution_backward(g, x, w, None, stride, padding, dilation, False, [0] * len(stride),
                                               groups, [True, False, False])[0]


# ---- pointwise (1x1, stride 1, unpadded) convolutions on channels_last activations as GEMMs
# An NHWC activation is a row-major [N*H*W, C] matrix, so a pointwise convolution is one GEMM
# (hipBLASLt) on a zero-copy view, and its input gradient is the GEMM with the weight untransposed.
# The forward's bias + ReLU run in the GEMM epilogue (torch._addmm_activation), so the fused
# ConvBiasReLU is a single kernel. Measured on MI355X at the c2 shapes (batch 832, bf16;
# scripts/gemm_probe.py, profiles/r01g_gemm_probe.log): 1.2-3.2x faster than the MIOpen
# convolution + epilogue pass forward, 1.1-1.9x faster for the input gradient.
# bf16 only: fp32 models keep the MIOpen convolutions, because the fp32 GEMM solution hipBLASLt
# picks varies by box in accumulation precision (one MI355X box gave a 3.4e-3 median relative
# input-gradient error on ResNet-50 NHWC against 1e-6 for the convolution path, r02h).
def _pointwise(w, geom):
    stride, padding, dilation, groups = geom
    return (w.dtype == torch.bfloat16 and w.dim() == 4 and w.shape[2] == 1 and w.shape[3] == 1 and groups == 1 and list(stride) == [1, 1]
            and list(padding) == [0, 0])


def _rows(t):
    """[N*H*W, C] view of a dense channels_last 4D tensor, or None."""
    if t.dim() != 4 or not t.is_cuda:
        return None
    v = t.permute(0, 2, 3, 1)
    return v.reshape(-1, t.shape[1]) if v.is_contiguous() else None


def _unrows(y2, like):
    n, _, h, w = like.shape
    return y2.view(n, h, w, y2.shape[1]).permute(0, 3, 1, 2)


def _addmm_relu(b, x2, w2t):
    try:
        return torch._addmm_activation(b, x2, w2t)
    except (AttributeError, RuntimeError):  # private op missing / no fused epilogue for this dtype
        return torch.relu_(torch.addmm(b, x2, w2t))


# ---- the expanding pointwise GEMM with its elementwise neighbour as the epilogue (csrc/model_pw.hip)
_PW_TAIL, _PW_MASK = 0, 1
# the model's launches round the accumulator to bf16 before the epilogue: the fused launch then
# computes what torch.mm followed by the wam_ew_* pass computes (the c2 maps of the two-kernel path bit
# for bit, profiles/r07b_dump_compare.log); applied to the unrounded accumulator the random-init bf16
# ResNet-50's ReLU masks flip and the maps move by 8e-2 relative L2
_PW_ROUNDED = 16
_PW_BITS = 32  # r1 is the packed ReLU mask of [M, N]: PW_TAIL writes it, PW_MASK reads it in place of y
# (mode, K, N) served by the fused kernel: the pairs that beat torch.mm + the wam_ew_* pass on
# MI355X (scripts/kbench_pointwise.py); anything else stays on the two-kernel path
_PW_ROUTES = {(_PW_TAIL, 64, 256), (_PW_TAIL, 128, 512), (_PW_MASK, 64, 256), (_PW_MASK, 128, 512)}


def _pw_routed(mode, w2):
    n, k = w2.shape
    return (mode, k, n) in _PW_ROUTES and w2.is_contiguous() and bool(_lib.lib.wam_pw_supported(_DT[w2.dtype], k, n))


def pw_gemm(mode, x2, w2, ba=None, bs=None, r0=None, r1=None):
    """epilogue(x2 [M, K] @ w2 [N, K]^T) -> [M, N]; PW_TAIL: r0 = s, PW_MASK: r0 = g2 or None, r1 = y.
    mode | _PW_BITS: r1 is the packed mask of [M, N] -- written by PW_TAIL, read for y by PW_MASK."""
    m, k = x2.shape
    n = w2.shape[0]
    out = torch.empty((m, n), dtype=x2.dtype, device=x2.device)
    cast = (lambda b: None if b is None else b.to(x2.dtype).contiguous())
    _lib.check(_lib.lib.wam_pw_gemm(mode | _PW_ROUNDED, _dt(x2), m, k, n, _lib.ptr(x2), _lib.ptr(w2), _lib.ptr(cast(ba)),
                                    _lib.ptr(cast(bs)), _lib.ptr(r0), _lib.ptr(r1), _lib.ptr(out), _stream(x2)))
    return out


class _PendingPW:
    """A ConvNoBias GEMM handed to the AddBiasReLU that consumes it, which runs it with the residual
    tail as its epilogue (one launch); any other consumer materialises it with today's mm."""

    __slots__ = ("x", "x2", "w2")

    def __init__(self, x, x2, w2):
        self.x, self.x2, self.w2 = x, x2, w2

    def materialize(self):
        return _PointwiseConvFn.apply(self.x2.detach(), self.x, self.w2)


class _SkipGrad:
    """Hand-off of a residual block's skip-path gradient to the block that produced its input.

    In a ResNet identity block the input x (the previous block's AddBiasReLU output) feeds both
    conv1 and the residual add, so autograd would sum the two gradients of x in a separate
    elementwise pass before the producer's ReLU mask (8 % of the c2 step). Instead the add
    receives x detached and parks its skip gradient here, and the producer's backward, which
    autograd runs later (it is upstream of both users), applies its mask to the sum in one kernel
    (relu_mask(g, y, g2)). One box per forward call: the producer's forward opens it and the
    consumer's forward takes it, so repeated forwards before a backward stay separate.

    Where the consumer block's conv1 runs on the GEMM path at a routed shape, its input-gradient
    GEMM takes the parked gradient and the producer's mask as its epilogue (PW_MASK: one launch
    instead of mm + relu_mask, 0.67-0.68x the pair's time at the c2 shapes) and
    marks the box `final`; the producer's backward then passes that gradient on as it is. `armed`
    says the consumer add took the box, i.e. a skip gradient will be parked. torch.addmm cannot
    do this: it copies its C operand into the output first (scripts/skip_ab.py)."""

    __slots__ = ("g", "armed", "final", "bits", "cl")

    def __init__(self):
        self.g = None
        self.armed = False
        self.final = False
        self.bits = None  # the producer's packed mask and its layout, for a _GradForkFn on its output
        self.cl = False


class _SkipLink:
    """Link between a producer AddBiasReLU and the consumer AddBiasReLU that takes its output as
    the skip operand."""

    def __init__(self):
        self.cur = None


def _masked_sum(take, g, out, bits=None, cl=False):
    """The producer's ReLU mask over g + the parked skip gradient -- or g as it is when the consumer's
    conv1 backward (PW_MASK) or the fork on the producer's output already applied both and marked
    the box final. The mask is the packed one (bits, cl) where the producer wrote it, else out > 0."""
    g2 = None
    if take is not None:
        if take.final:
            take.final = False
            return _dense(g, cl) if bits is not None else _like(g, out)
        g2, take.g = take.g, None
    if bits is not None:
        return relu_mask_bits(g, bits, cl, g2)
    return relu_mask(g, out, g2)


class _ConvBiasReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, geom, box=None, wt=None):
        x2 = _rows(x) if _pointwise(w, geom) else None
        ctx.gemm = x2 is not None
        ctx.box = None
        if ctx.gemm:
            w2 = w.reshape(w.shape[0], w.shape[1])
            y = _unrows(_addmm_relu(b.to(x.dtype), x2, w2.t()), x)
            if box is not None and wt is not None and x.dtype == w.dtype:
                # x is the linked producer's output: its mask and the skip gradient parked in the
                # box become the epilogue of this convolution's input-gradient GEMM
                ctx.box = box
                ctx.xbits, ctx.xshape = box.bits is not None, x.shape
                ctx.save_for_backward(w2, y, wt, box.bits if ctx.xbits else x)
            else:
                ctx.save_for_backward(w2, y)
            return y
        y, bits = bias_relu_bits_(_conv_nd(x, w, *geom), b)
        ctx.cl = bits is not None and _is_cl(y)  # with the packed mask, y itself is not kept
        ctx.save_for_backward(x, w, y if bits is None else bits)
        ctx.geom, ctx.bits = geom, bits is not None
        return y

    @staticmethod
    def backward(ctx, g):
        if ctx.gemm:
            w2, y = ctx.saved_tensors[:2]
            gm = relu_mask(g, y)
            box = ctx.box
            if box is not None and box.armed:
                wt, x = ctx.saved_tensors[2:]
                # the consumer's tail runs before this backward (_link_skip_gradients), so its skip
                # gradient is parked by now; a missing one would silently drop a gradient branch
                if box.g is None:
                    raise RuntimeError("wam_amd: the skip gradient of a linked residual block was not parked "
                                       "before its conv1 backward")
                g2 = _rows(box.g)
                if g2 is not None and g2.dtype == gm.dtype:
                    box.g, box.final = None, True
                    if ctx.xbits:  # x holds the producer's packed mask, not its output
                        dx = pw_gemm(_PW_MASK | _PW_BITS, _rows(gm), wt, None, None, g2, x)
                    else:
                        dx = pw_gemm(_PW_MASK, _rows(gm), wt, None, None, g2, _rows(x))
                    n, _, h, ww = ctx.xshape
                    return dx.view(n, h, ww, dx.shape[1]).permute(0, 3, 1, 2), None, None, None, None, None
            return _unrows(torch.mm(_rows(gm), w2), y), None, None, None, None, None
        x, w, y = ctx.saved_tensors
        gm = relu_mask_bits(g, y, ctx.cl) if ctx.bits else relu_mask(g, y)
        return _conv_grad_input(gm, x, w, *ctx.geom), None, None, None, None, None


class _PointwiseConvFn(torch.autograd.Function):
    """Bias-free pointwise convolution of a channels_last activation as a GEMM."""

    @staticmethod
    def forward(ctx, x2, x, w2):
        ctx.save_for_backward(w2)
        ctx.shape = x.shape
        y = torch.mm(x2, w2.t())
        n, _, h, ww = x.shape
        return y.view(n, h, ww, w2.shape[0]).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        (w2,) = ctx.saved_tensors
        g2 = _rows(g)
        if g2 is None:
            g2 = _rows(g.contiguous(memory_format=torch.channels_last))
        n, c, h, ww = ctx.shape
        dx = torch.mm(g2, w2).view(n, h, ww, c).permute(0, 3, 1, 2)
        return None, dx, None


class _AddBiasReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, ba, s, bs, park=None, take=None):
        out, bits = add_bias_relu_bits(a, ba, s, bs)
        ctx.cl = bits is not None and _is_cl(out)
        ctx.save_for_backward(out if bits is None else bits)
        ctx.park, ctx.take, ctx.bits = park, take, bits is not None
        if take is not None:
            take.bits, take.cl = bits, ctx.cl
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        # skip gradient of the consumer block, summed under the mask
        gm = _masked_sum(ctx.take, g, out, out if ctx.bits else None, ctx.cl)
        if ctx.park is not None:  # s was passed detached: its gradient goes to s's producer
            ctx.park.g = gm
            return gm, None, None, None, None, None
        return gm, None, gm, None, None, None


class _PWTailFn(torch.autograd.Function):
    """relu((conv1x1(x, w2) + ba) + (s + bs)) in one launch. Backward = _AddBiasReLUFn's mask pass,
    then _PointwiseConvFn's input-gradient GEMM for the convolution branch."""

    @staticmethod
    def forward(ctx, x, w2, ba, s, bs, park=None, take=None):
        bits = _new_bits(s) if _bits_ok(s) else None
        if bits is None:
            out = _unrows(pw_gemm(_PW_TAIL, _rows(x), w2, ba, bs, _rows(s)), s)
        else:
            out = _unrows(pw_gemm(_PW_TAIL | _PW_BITS, _rows(x), w2, ba, bs, _rows(s), bits), s)
        ctx.cl = bits is not None and _is_cl(out)
        ctx.save_for_backward(w2, out if bits is None else bits)
        ctx.park, ctx.take, ctx.bits, ctx.shape = park, take, bits is not None, out.shape
        if take is not None:
            take.bits, take.cl = bits, ctx.cl
        return out

    @staticmethod
    def backward(ctx, g):
        w2, out = ctx.saved_tensors
        gm = _masked_sum(ctx.take, g, out, out if ctx.bits else None, ctx.cl)
        n, _, h, ww = ctx.shape
        dx = torch.mm(_rows(gm), w2).view(n, h, ww, w2.shape[1]).permute(0, 3, 1, 2)
        if ctx.park is not None:
            ctx.park.g = gm
            return dx, None, None, None, None, None, None
        return dx, None, None, gm, None, None, None


class _GradForkFn(torch.autograd.Function):
    """A fused tail's output handed to its two users (a downsample block's conv1 and its shortcut
    convolution) as two outputs, so that the backward receives both gradients -- autograd calls it
    only when both have arrived -- and runs the producer's ReLU mask over their sum in ONE launch:
    without it autograd sums them with a torch add (3 passes) before the producer's mask (3 passes).
    bf16(g1 + g2) rounds once either way and the mask only selects, so the bits are the same. The
    box is marked final: the producer's backward passes the result on as it is."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        ctx.bits, ctx.cl = box.bits is not None, box.cl
        ctx.save_for_backward(box.bits if ctx.bits else x)
        ctx.set_materialize_grads(False)
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is None:
            g1, g2 = g2, None
        if g1 is None:
            return None, None
        (y,) = ctx.saved_tensors
        gm = relu_mask_bits(g1, y, ctx.cl, g2) if ctx.bits else relu_mask(g1, y, g2)
        ctx.box.final = True
        return gm, None


class _PolyphaseReLUFn(torch.autograd.Function):
    """relu(InputConv2d(x)): conv without bias + fused bias/ReLU; backward = mask + polyphase."""

    @staticmethod
    def forward(ctx, x, weight, bias, wpoly, pad, geom):
        y = bias_act_(F.conv2d(x, weight, None, 2, pad), bias, True)
        ctx.save_for_backward(wpoly, y)
        ctx.geom = geom
        ctx.in_hw = x.shape[-2:]
        return y

    @staticmethod
    def backward(ctx, go):
        wpoly, y = ctx.saved_tensors
        gm = relu_mask(go, y)

        class _C:  # reuse the polyphase backward with its saved table
            saved_tensors = (wpoly,)
            geom = ctx.geom
            in_hw = ctx.in_hw
        return _PolyphaseInputGrad.backward(_C, gm)


class _PolyphaseReLUPoolFn(torch.autograd.Function):
    """maxpool(relu(InputConv2d(x))): the pooled input is not kept -- the byte window index
    carries the ReLU mask, so the backward is one gather kernel + the polyphase convolution."""

    @staticmethod
    def forward(ctx, x, weight, bias, wpoly, pad, geom, pool):
        y = F.conv2d(x, weight, None, 2, pad)
        k, s, p = pool
        ctx.geom, ctx.in_hw, ctx.pool, ctx.y_shape = geom, x.shape[-2:], pool, y.shape
        # the pool applies bias + ReLU to what it loads: the biased tensor is never written
        fused = bias_relu_maxpool_nhwc(y, bias, k, s, p) if RELU_BITS and _pool_ok(y, k, s, p) else None
        if fused is not None:
            ctx.save_for_backward(wpoly, fused[1])
            ctx.hip = True
            return fused[0]
        y = bias_act_(y, bias, True)
        if _pool_ok(y, k, s, p):
            out, idx = maxpool_nhwc(y, k, s, p)
            ctx.save_for_backward(wpoly, idx)
            ctx.hip = True
        else:
            out, idx = F.max_pool2d(y, k, s, p, return_indices=True)
            ctx.save_for_backward(wpoly, idx, y)
            ctx.hip = False
        return out

    @staticmethod
    def backward(ctx, go):
        k, s, p = ctx.pool
        if ctx.hip:
            wpoly, idx = ctx.saved_tensors
            gm = maxpool_nhwc_backward(go, idx, ctx.y_shape, k, s, p, relu=True)
        else:
            wpoly, idx, y = ctx.saved_tensors
            gy = torch.ops.aten.max_pool2d_with_indices_backward(go, y, [k, k], [s, s], [p, p], [1, 1], False, idx)
            gm = relu_mask(gy, y)

        class _C:  # reuse the polyphase backward with its saved table
            saved_tensors = (wpoly,)
            geom = ctx.geom
            in_hw = ctx.in_hw
        return _PolyphaseInputGrad.backward(_C, gm) + (None,)


def _geom(conv):
    return (list(conv.stride), list(conv.padding), list(conv.dilation), conv.groups)


class ConvBiasReLU(nn.Module):
    """relu(conv(x)) for a frozen, zero-padded Conv1d/2d/3d with bias (one fused epilogue)."""

    def __init__(self, conv):
        super().__init__()
        self.weight = nn.Parameter(conv.weight.detach().clone(), requires_grad=False)
        b = conv.bias.detach().clone() if conv.bias is not None else torch.zeros(conv.out_channels)
        self.bias = nn.Parameter(b, requires_grad=False)
        self.geom = _geom(conv)
        self.link_src = None  # _SkipLink: the input is a linked producer's output (fused mask backward)
        self._wt = self._wt_key = None

    def _weight_t(self):
        """[C_in, C_out] copy of the frozen pointwise weight (PW_MASK's w operand), made once."""
        w = self.weight
        key = (w.data_ptr(), w.dtype, w.device, w._version)
        if self._wt_key != key:
            self._wt, self._wt_key = w.reshape(w.shape[0], w.shape[1]).t().contiguous(), key
        return self._wt

    def forward(self, x):
        box = wt = None
        if self.link_src is not None and self.link_src.cur is not None and torch.is_grad_enabled() and x.is_cuda \
                and _pointwise(self.weight, self.geom) and x.dtype == self.weight.dtype \
                and (_PW_MASK, self.weight.shape[0], self.weight.shape[1]) in _PW_ROUTES:
            wt = self._weight_t()
            if _pw_routed(_PW_MASK, wt):
                box = self.link_src.cur
        return _ConvBiasReLUFn.apply(x, self.weight, self.bias, self.geom, box, wt)


class ConvNoBias(nn.Module):
    """conv(x) with its bias moved into the consumer (AddBiasReLU)."""

    def __init__(self, conv):
        super().__init__()
        self.weight = nn.Parameter(conv.weight.detach().clone(), requires_grad=False)
        self.geom = _geom(conv)
        self.defer = False  # its only user is an AddBiasReLU's `a` operand, which can run the GEMM itself

    def forward(self, x):
        if _pointwise(self.weight, self.geom):
            x2 = _rows(x)
            if x2 is not None:
                w2 = self.weight.reshape(self.weight.shape[0], self.weight.shape[1])
                if self.defer and x.dtype == w2.dtype and _pw_routed(_PW_TAIL, w2):
                    return _PendingPW(x, x2, w2)
                return _PointwiseConvFn.apply(x2.detach(), x, w2)
        return _conv_nd(x, self.weight, *self.geom)


class AddBiasReLU(nn.Module):
    """relu((a + bias_a) + (s + bias_s)) -- residual tail; biases may be absent."""

    def __init__(self, bias_a=None, bias_s=None):
        super().__init__()
        self.bias_a = None if bias_a is None else nn.Parameter(bias_a.detach().clone(), requires_grad=False)
        self.bias_s = None if bias_s is None else nn.Parameter(bias_s.detach().clone(), requires_grad=False)

        self.link_in = None   # _SkipLink: operand s comes from a linked producer (park its gradient)
        self.link_out = None  # _SkipLink: this output is a linked consumer's skip operand (take it)
        self.fork_out = None  # _SkipLink: this output goes through a GradFork (it applies this mask)

    def _fusable(self, a, s):
        """The HIP kernel indexes s with a's flat index: same shape, dtype, layout and device only."""
        if not (a.is_cuda and s.is_cuda and a.device == s.device and a.dtype == s.dtype and a.dtype in _DT
                and a.shape == s.shape and a.dim() >= 2):
            return False
        for b in (self.bias_a, self.bias_s):
            if b is not None and (b.dim() != 1 or b.numel() != a.shape[1]):
                return False
        return True

    def _pending_ok(self, p, s):
        """The fused GEMM writes [M, N] rows next to s's rows: s dense channels_last of the output's shape."""
        x = p.x
        if not (isinstance(s, torch.Tensor) and s.is_cuda and s.device == x.device and s.dtype == x.dtype
                and tuple(s.shape) == (x.shape[0], p.w2.shape[0], x.shape[2], x.shape[3]) and _rows(s) is not None):
            return False
        for b in (self.bias_a, self.bias_s):
            if b is not None and (b.dim() != 1 or b.numel() != s.shape[1]):
                return False
        return True

    def forward(self, a, s):
        pending = None
        if isinstance(a, _PendingPW):
            if self._pending_ok(a, s):
                pending, a = a, a.x
            else:
                a = a.materialize()
        if pending is None and not self._fusable(a, s):
            # broadcast / mixed operands (e.g. relu(x + pos_embed)): plain torch, no skip hand-off
            if self.link_out is not None:
                self.link_out.cur = None
            if self.link_in is not None:
                self.link_in.cur = None
            if self.fork_out is not None:
                self.fork_out.cur = None
            bias = (lambda t, b: t if b is None else t + b.to(t.dtype).view((1, -1) + (1,) * (t.dim() - 2)))
            return torch.relu(bias(a, self.bias_a) + bias(s, self.bias_s))
        park = take = None
        if self.link_in is not None and self.link_in.cur is not None and torch.is_grad_enabled():
            park, self.link_in.cur = self.link_in.cur, None
            park.armed = True
            s = s.detach()
        if self.link_out is not None:
            grad = torch.is_grad_enabled() and (a.requires_grad or s.requires_grad)
            take = self.link_out.cur = _SkipGrad() if grad else None
        elif self.fork_out is not None:
            grad = RELU_BITS and torch.is_grad_enabled() and (a.requires_grad or s.requires_grad)
            take = self.fork_out.cur = _SkipGrad() if grad else None
        if pending is not None:
            return _PWTailFn.apply(a, pending.w2, self.bias_a, s, self.bias_s, park, take)
        return _AddBiasReLUFn.apply(a, self.bias_a, s, self.bias_s, park, take)


class GradFork(nn.Module):
    """x -> (x, x) for the two users of a fused tail's output at a downsample junction; with grad on
    a CUDA tensor the pair comes from _GradForkFn, whose backward fuses the gradient sum into the
    producer's ReLU mask. Anything else (no grad, CPU, an unfused producer) gets x twice."""

    def __init__(self):
        super().__init__()
        self.src = None  # _SkipLink to the producing AddBiasReLU (its fork_out)

    def forward(self, x):
        box = None
        if self.src is not None:
            box, self.src.cur = self.src.cur, None
        if box is None or not torch.is_grad_enabled() or not x.is_cuda or not x.requires_grad:
            return x, x
        return _GradForkFn.apply(x, box)


class InputConvReLU(nn.Module):
    """relu(InputConv2d(x)) with the fused bias/ReLU epilogue and masked polyphase backward."""

    def __init__(self, ic):
        super().__init__()
        self.ic = ic

    def forward(self, x):
        from .model_opt import _phase_geometry
        ic = self.ic
        H, W = x.shape[-2:]
        oy, Ty, _, ny = _phase_geometry(ic.kh, ic.pad[0], H)
        ox, Tx, _, nx = _phase_geometry(ic.kw, ic.pad[1], W)
        b = ic.bias if ic.bias is not None else torch.zeros(ic.weight.shape[0], dtype=ic.weight.dtype,
                                                            device=ic.weight.device)
        return _PolyphaseReLUFn.apply(x, ic.weight, b, ic.wpoly, ic.pad, ((oy, Ty, ny), (ox, Tx, nx)))


class InputConvReLUPool(InputConvReLU):
    """maxpool(relu(InputConv2d(x))) for a square, undilated, floor-mode max pool."""

    def __init__(self, ic, pool):
        super().__init__(ic)
        self.pool = pool  # (k, stride, pad)

    def forward(self, x):
        from .model_opt import _phase_geometry
        ic = self.ic
        H, W = x.shape[-2:]
        oy, Ty, _, ny = _phase_geometry(ic.kh, ic.pad[0], H)
        ox, Tx, _, nx = _phase_geometry(ic.kw, ic.pad[1], W)
        b = ic.bias if ic.bias is not None else torch.zeros(ic.weight.shape[0], dtype=ic.weight.dtype,
                                                            device=ic.weight.device)
        return _PolyphaseReLUPoolFn.apply(x, ic.weight, b, ic.wpoly, ic.pad, ((oy, Ty, ny), (ox, Tx, nx)), self.pool)


def _square(v):
    if isinstance(v, (tuple, list)):
        return v[0] if len(set(v)) == 1 else None
    return v


def _simple_pool(m):
    """(k, stride, pad) of a MaxPool2d the fused kernels implement, or None."""
    if type(m) is not nn.MaxPool2d or m.ceil_mode or m.return_indices or _square(m.dilation) != 1:
        return None
    k, s, p = _square(m.kernel_size), _square(m.stride if m.stride is not None else m.kernel_size), _square(m.padding)
    if None in (k, s, p) or 2 * p > k or k * k > 127:
        return None
    return (int(k), int(s), int(p))


# --------------------------------------------------------------------------------- graph rewrite
_RELU_FN = (F.relu, torch.relu)


def _is_relu(node, mods):
    if node.op == "call_module":
        m = mods.get(node.target)
        return type(m) is nn.ReLU
    if node.op == "call_function":
        return node.target in _RELU_FN and len(node.args) == 1
    if node.op == "call_method":
        return node.target in ("relu", "relu_") and len(node.args) == 1
    return False


def _fusable_conv(node, mods):
    if node.op != "call_module" or len(node.users) != 1:
        return None
    m = mods.get(node.target)
    if type(m) in (nn.Conv1d, nn.Conv2d, nn.Conv3d) and m.padding_mode == "zeros" and not isinstance(m.padding, str):
        return m
    return None


def fuse_elementwise(gm):
    """Rewrite a traced (BN-folded, frozen) GraphModule in place; returns it and the fusion count."""
    mods = dict(gm.named_modules())
    g = gm.graph
    count = 0
    uid = [0]

    def add_mod(prefix, m):
        uid[0] += 1
        name = "%s_wamfuse%d" % (prefix.replace(".", "_"), uid[0])
        gm.add_submodule(name, m)
        mods[name] = m
        return name

    for node in list(g.nodes):
        if not _is_relu(node, mods):
            continue
        src = node.args[0]
        if not isinstance(src, fx.Node) or len(src.users) != 1:
            continue
        conv = _fusable_conv(src, mods)
        if conv is not None:  # conv -> relu
            name = add_mod(src.target, ConvBiasReLU(conv))
            with g.inserting_before(node):
                new = g.call_module(name, (src.args[0],))
            node.replace_all_uses_with(new)
            g.erase_node(node)
            g.erase_node(src)
            count += 1
            continue
        if src.op == "call_module" and isinstance(mods.get(src.target), InputConv2d):  # input conv -> relu
            name = add_mod(src.target, InputConvReLU(mods[src.target]))
            with g.inserting_before(node):
                new = g.call_module(name, (src.args[0],))
            node.replace_all_uses_with(new)
            g.erase_node(node)
            g.erase_node(src)
            count += 1
            continue
        if src.op == "call_function" and src.target in (operator.add, torch.add) and len(src.args) == 2 \
                and not src.kwargs and all(isinstance(a, fx.Node) for a in src.args):
            operands, biases, drop = [], [], []
            for a in src.args:
                c = _fusable_conv(a, mods)
                if c is not None and c.bias is not None:
                    cname = add_mod(a.target, ConvNoBias(c))
                    mods[cname].defer = a is src.args[0]
                    with g.inserting_before(a):
                        na = g.call_module(cname, (a.args[0],))
                    operands.append(na)
                    biases.append(c.bias)
                    drop.append(a)
                else:
                    operands.append(a)
                    biases.append(None)
            name = add_mod("add_relu", AddBiasReLU(*biases))
            with g.inserting_before(node):
                new = g.call_module(name, tuple(operands))
            node.replace_all_uses_with(new)
            g.erase_node(node)
            g.erase_node(src)
            for a in drop:
                g.erase_node(a)
            count += 1
    for node in list(g.nodes):  # stem relu -> max pool
        if node.op != "call_module" or _simple_pool(mods.get(node.target)) is None:
            continue
        src = node.args[0] if node.args else None
        if not isinstance(src, fx.Node) or src.op != "call_module" or len(src.users) != 1 \
                or type(mods.get(src.target)) is not InputConvReLU:
            continue
        name = add_mod(src.target, InputConvReLUPool(mods[src.target].ic, _simple_pool(mods[node.target])))
        with g.inserting_before(node):
            new = g.call_module(name, (src.args[0],))
        node.replace_all_uses_with(new)
        g.erase_node(node)
        g.erase_node(src)
        count += 1
    _link_skip_gradients(gm, mods)
    _fork_junction_gradients(gm, mods, add_mod)
    g.lint()
    gm.recompile()
    gm.delete_all_unused_submodules()
    return gm, count


def _reaches(src, dst):
    """True when fx node dst is src or one of its (transitive) users."""
    seen, stack = set(), [src]
    while stack:
        n = stack.pop()
        if n is dst:
            return True
        if n in seen:
            continue
        seen.add(n)
        stack.extend(n.users)
    return False


def _descendants(src):
    """src and every fx node that uses it, directly or not."""
    seen, stack = set(), [src]
    while stack:
        n = stack.pop()
        if n not in seen:
            seen.add(n)
            stack.extend(n.users)
    return seen


def _link_skip_gradients(gm, mods):
    """Link each identity residual block's AddBiasReLU with the AddBiasReLU that produced its skip
    operand, when that output has exactly two users: the block's conv1 and the add (_SkipGrad)."""
    links = 0
    for node in gm.graph.nodes:
        if node.op != "call_module" or type(mods.get(node.target)) is not AddBiasReLU:
            continue
        users = list(node.users)
        if len(users) != 2:
            continue
        add = [u for u in users if u.op == "call_module" and type(mods.get(u.target)) is AddBiasReLU]
        if len(add) != 1 or len(add[0].args) != 2 or add[0].args[1] is not node or add[0].args[0] is node:
            continue
        # the parked gradient is only complete if autograd runs the consumer before the producer:
        # true when the producer's other user feeds the consumer's `a` operand (then the
        # consumer's backward precedes every gradient that reaches the producer through it)
        other = [u for u in users if u is not add[0]]
        if len(other) != 1 or not _reaches(other[0], add[0].args[0]):
            continue
        link = _SkipLink()
        mods[node.target].link_out = link
        mods[add[0].target].link_in = link
        if type(mods.get(other[0].target)) is ConvBiasReLU and other[0].args[0] is node:
            mods[other[0].target].link_src = link  # the block's conv1: fused mask backward
        links += 1
    return links


def _fork_junction_gradients(gm, mods, add_mod):
    """Route each AddBiasReLU output with exactly two users whose branches meet, one per operand, in
    the nearest later AddBiasReLU (a downsample block: conv1 towards operand a, the shortcut
    convolution towards s) through a GradFork. The identity-skip pattern (one user IS the add) is
    _link_skip_gradients' and is left alone. Not a fusion of forward nodes, so it is not counted as
    one. (The fork itself is right for any two users: it only sums two gradients under the
    producer's mask; the pattern keeps it to the junctions it was measured on.)"""
    g = gm.graph
    forks = 0
    order = [n for n in g.nodes if n.op == "call_module"]
    for node in list(order):
        if type(mods.get(node.target)) is not AddBiasReLU:
            continue
        users = list(node.users)
        if len(users) != 2 or mods[node.target].link_out is not None:
            continue
        if any(u.op != "call_module" or type(mods.get(u.target)) is AddBiasReLU for u in users):
            continue
        if any(sum(a is node for a in u.all_input_nodes) != 1 or u.kwargs for u in users):
            continue
        # the nearest junction: the first AddBiasReLU (graph order is topological) that either branch
        # reaches has to take one branch per operand
        below = [_descendants(u) for u in users]
        join = next((j for j in order[order.index(node) + 1:]
                     if type(mods.get(j.target)) is AddBiasReLU and (j in below[0] or j in below[1])), None)
        if join is None or len(join.args) != 2 or not all(isinstance(a, fx.Node) for a in join.args):
            continue
        a, b = join.args
        if not ((a in below[0] and b in below[1]) or (a in below[1] and b in below[0])):
            continue
        link = _SkipLink()
        fork = GradFork()
        fork.src = link
        mods[node.target].fork_out = link
        name = add_mod("grad_fork", fork)
        with g.inserting_after(node):
            f = g.call_module(name, (node,))
        with g.inserting_after(f):
            outs = [g.call_function(operator.getitem, (f, i)) for i in (1, 0)][::-1]
        for u, o in zip(users, outs):
            u.replace_input_with(node, o)
        forks += 1
    return forks
