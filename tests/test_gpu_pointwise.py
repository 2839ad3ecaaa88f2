"""The weight-stationary pointwise GEMM with a fused epilogue (wam_amd/csrc/model_pw.hip) at the C
ABI against a float64 torch reference built from the same bf16 inputs, and the model path that
uses it (wam_amd/model_fuse.py: conv3 + residual tail as one launch, conv1's input gradient + the
producer's ReLU mask as one launch).

Tolerance (kernel tests): only the fp32 accumulation order and the final bf16 rounding separate the
kernel from the reference, so elementwise
    |got - ref| <= 2^-7 |ref| + K 2^-23 (|X| |W|^T + |ba| + |bs| + |s|)
with the second term evaluated in float64 from the absolute values (|g2| takes the place of |s| in
the mask mode). Every element of every case has to pass.

With WAM_PW_ROUNDED (the form the model launches: the accumulator is rounded to bf16 before the
epilogue, as the bf16 GEMM of the two-kernel path rounds its result) the value the epilogue sees
differs from the exact product by at most half a bf16 ulp, 2^-8 |acc| (8 significand bits), plus
the fp32 accumulation error already in the second term; the epilogue is 1-Lipschitz in acc, so
that form is held to the bound above plus 2^-8 (1 + 2^-8) |X . W^T|.
"""
import functools

import pytest
import torch
import torch.nn as nn

import testmodels
from wam_amd.model_opt import optimize_for_input_grad

SHAPES = [(64, 256), (128, 512)]
ROWS = [1, 30, 49, 257, 2 * 56 * 56 + 3]
TAIL, MASK, ROUNDED = 0, 1, 16
BF16 = 1
UNSUPPORTED, INVALID = 3, 1


def _lib():
    from wam_amd import _lib
    return _lib


def _stream():
    return _lib().c_vp(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(None)
def _case(K, N, M):
    """bf16 operands of one (K, N, M) and the float64 products every test of that shape shares."""
    g = torch.Generator(device="cuda").manual_seed(1000 * K + M)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    uni = lambda *s: torch.rand(*s, device="cuda", generator=g)  # noqa: E731
    x = rnd(M, K).bfloat16()
    w = (rnd(N, K) / K ** 0.5).bfloat16()
    ba, bs = rnd(N).bfloat16(), rnd(N).bfloat16()
    # s: exact zeros (20 %) and a negative offset, so that about half of the sums clamp
    s = (1.5 * rnd(M, N) - 0.4).bfloat16()
    s = torch.where(uni(M, N) < 0.2, torch.zeros_like(s), s)
    g2 = rnd(M, N).bfloat16()
    # y: a ReLU output with 30 % exact zeros (as the max-pool test), plus -0.0 and NaN entries
    y = rnd(M, N).bfloat16()
    u = uni(M, N)
    y = torch.where(u < 0.3, torch.zeros_like(y), y)
    y = torch.where((u >= 0.3) & (u < 0.33), torch.full_like(y, -0.0), y)
    y = torch.where((u >= 0.33) & (u < 0.36), torch.full_like(y, float("nan")), y)
    acc = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    return dict(x=x, w=w, ba=ba, bs=bs, s=s, g2=g2, y=y, acc=acc, mag=mag)


def _run(mode, K, N, M, x, w, ba, bs, r0, r1, cap=None, out=None):
    L = _lib()
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16) if out is None else out
    p = L.ptr
    if cap is None:
        rc = L.lib.wam_pw_gemm(mode, BF16, M, K, N, p(x), p(w), p(ba), p(bs), p(r0), p(r1), p(out), _stream())
    else:
        rc = L.lib.wam_pw_gemm_ex(mode, M, K, N, p(x), p(w), p(ba), p(bs), p(r0), p(r1), p(out), cap, _stream())
    torch.cuda.synchronize()
    return rc, out


def _check(got, ref, slack, K, what, rounded_acc=None):
    tol = 2.0 ** -7 * ref.abs() + K * 2.0 ** -23 * slack
    if rounded_acc is not None:  # WAM_PW_ROUNDED: half a bf16 ulp of the accumulator (module docstring)
        tol = tol + 2.0 ** -8 * (1 + 2.0 ** -8) * rounded_acc.abs()
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)  # a NaN in got fails
    assert not bool(bad.any()), "%s: %d of %d outside the tolerance, worst excess %.3g" % (
        what, int(bad.sum()), bad.numel(), float((err - tol)[bad].max()))


def _caps(M):
    # the grid follows the CU count; 3 workgroups make 6,275 rows loop >= 8 times in every workgroup
    return [None, 3] if M > 1000 else [None]


@pytest.mark.gpu
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_gpu_pw_tail_matches_float64(K, N, M):
    c = _case(K, N, M)
    z = torch.zeros(N, device="cuda", dtype=torch.float64)
    for use_a, use_s in [(True, True), (True, False), (False, True), (False, False)]:
        ba, bs = (c["ba"] if use_a else None), (c["bs"] if use_s else None)
        da, ds = (ba.double() if use_a else z), (bs.double() if use_s else z)
        pre = (c["acc"] + da) + (c["s"].double() + ds)
        ref = pre.clamp_min(0)
        if use_a and use_s:
            frac = float((pre <= 0).double().mean())
            assert 0.3 < frac < 0.7, frac  # about half of the outputs clamp
        slack = c["mag"] + da.abs() + ds.abs() + c["s"].double().abs()
        for cap in _caps(M):
            rc, got = _run(TAIL, K, N, M, c["x"], c["w"], ba, bs, c["s"], None, cap)
            assert rc == 0
            _check(got, ref, slack, K, "tail K=%d M=%d ba=%s bs=%s cap=%s" % (K, M, use_a, use_s, cap))
            rc, got = _run(TAIL | ROUNDED, K, N, M, c["x"], c["w"], ba, bs, c["s"], None, cap)
            assert rc == 0
            _check(got, ref, slack, K, "rounded tail K=%d M=%d ba=%s bs=%s cap=%s" % (K, M, use_a, use_s, cap),
                   c["acc"])
    # the same case with NaN entries in s and a NaN row in x: the forward ReLU passes NaN on (as
    # torch.relu and the unfused model do), so the output is NaN at exactly the reference's elements
    # and every other element is held to the bound above
    g = torch.Generator(device="cuda").manual_seed(7 * K + M)
    s = torch.where(torch.rand(M, N, device="cuda", generator=g) < 0.03, torch.full_like(c["s"], float("nan")), c["s"])
    s[0, 0] = float("nan")
    x = c["x"].clone()
    x[M // 2] = float("nan")
    pre = (x.double() @ c["w"].double().t() + c["ba"].double()) + (s.double() + c["bs"].double())
    nan = torch.isnan(pre)
    assert bool(nan[M // 2].all()) and bool(nan[0, 0]) and (M < 30 or not bool(nan.all()))
    fin = lambda t: torch.where(nan, torch.zeros_like(t), t)  # noqa: E731
    ref = fin(pre).clamp_min(0)
    slack = fin(x.double().abs() @ c["w"].double().abs().t()) + c["ba"].double().abs() + c["bs"].double().abs() \
        + fin(s.double().abs())
    for cap in _caps(M):
        for mode in (TAIL, TAIL | ROUNDED):
            rc, got = _run(mode, K, N, M, x, c["w"], c["ba"], c["bs"], s, None, cap)
            assert rc == 0
            assert torch.equal(torch.isnan(got), nan), "tail mode %d K=%d M=%d cap=%s: %d NaN outputs, reference %d" % (
                mode, K, M, cap, int(torch.isnan(got).sum()), int(nan.sum()))
            _check(fin(got), ref, slack, K, "tail with NaN inputs, mode %d K=%d M=%d cap=%s" % (mode, K, M, cap),
                   fin(x.double() @ c["w"].double().t()) if mode & ROUNDED else None)


@pytest.mark.gpu
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_gpu_pw_mask_matches_float64(K, N, M):
    c = _case(K, N, M)
    y = c["y"]
    dead = ~(y > 0)  # zeros, -0.0, negatives and NaN: k_relu_mask's `y > 0 ? . : 0`
    assert bool((y == 0).any()) or M < 30
    for g2 in (c["g2"], None):
        pre = c["acc"] + (g2.double() if g2 is not None else 0)
        ref = torch.where(dead, torch.zeros_like(pre), pre)
        slack = c["mag"] + (g2.double().abs() if g2 is not None else 0)
        for cap in _caps(M):
            rc, got = _run(MASK, K, N, M, c["x"], c["w"], None, None, g2, y, cap)
            assert rc == 0
            assert bool((got[dead] == 0).all()), "mask mode: a non-zero output where y <= 0 / NaN"
            _check(got, ref, slack, K, "mask K=%d M=%d g2=%s cap=%s" % (K, M, g2 is not None, cap))
            rc, got = _run(MASK | ROUNDED, K, N, M, c["x"], c["w"], None, None, g2, y, cap)
            assert rc == 0
            assert bool((got[dead] == 0).all()), "rounded mask mode: a non-zero output where y <= 0 / NaN"
            _check(got, ref, slack, K, "rounded mask K=%d M=%d g2=%s cap=%s" % (K, M, g2 is not None, cap), c["acc"])


@pytest.mark.gpu
def test_gpu_pw_rejections_leave_out_untouched():
    L = _lib()
    assert L.lib.wam_pw_supported(BF16, 64, 256) == 1 and L.lib.wam_pw_supported(BF16, 128, 512) == 1
    assert L.lib.wam_pw_supported(BF16, 96, 256) == 0 and L.lib.wam_pw_supported(BF16, 64, 512) == 0
    assert L.lib.wam_pw_supported(0, 64, 256) == 0
    M = 49
    sentinel = 1.5
    mk = lambda *s: torch.randn(*s, device="cuda").bfloat16()  # noqa: E731
    p = L.ptr

    def call(mode, dtype, K, N, x, w, r0, r1, out):
        rc = L.lib.wam_pw_gemm(mode, dtype, M, K, N, x, p(w), None, None, p(r0), p(r1), p(out), _stream())
        torch.cuda.synchronize()
        return rc

    for K, N, dtype in [(96, 256, BF16), (64, 512, BF16), (64, 256, 0)]:
        x, w, s = mk(M, K), mk(N, K), mk(M, N)
        out = torch.full((M, N), sentinel, device="cuda", dtype=torch.bfloat16)
        assert call(TAIL, dtype, K, N, p(x), w, s, None, out) == UNSUPPORTED
        assert call(MASK, dtype, K, N, p(x), w, None, s, out) == UNSUPPORTED
        assert bool((out == sentinel).all())
    # an x pointer offset by one bf16 element (2 bytes)
    K, N = 64, 256
    xbuf, w, s = mk(M * K + 8), mk(N, K), mk(M, N)
    out = torch.full((M, N), sentinel, device="cuda", dtype=torch.bfloat16)
    assert call(TAIL, BF16, K, N, L.c_vp(xbuf.data_ptr() + 2), w, s, None, out) == UNSUPPORTED
    assert bool((out == sentinel).all())
    # invalid arguments: M <= 0, NULL x / w / out
    x = mk(M, K)
    assert L.lib.wam_pw_gemm(TAIL, BF16, 0, K, N, p(x), p(w), None, None, p(s), None, p(out), _stream()) == INVALID
    assert L.lib.wam_pw_gemm(TAIL, BF16, M, K, N, None, p(w), None, None, p(s), None, p(out), _stream()) == INVALID
    assert L.lib.wam_pw_gemm(TAIL, BF16, M, K, N, p(x), None, None, None, p(s), None, p(out), _stream()) == INVALID
    assert L.lib.wam_pw_gemm(TAIL, BF16, M, K, N, p(x), p(w), None, None, p(s), None, None, _stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


# ------------------------------------------------------------------------------------ model level
def _stage2_stack(seed=0):
    """ResNet-50's first bottleneck stage: 3 blocks of widths 64 -> 256, the first with a downsample."""
    torch.manual_seed(seed)
    down = nn.Sequential(nn.Conv2d(64, 256, 1, 1, bias=False), nn.BatchNorm2d(256))
    net = nn.Sequential(testmodels.Bottleneck(64, 64, 1, down), testmodels.Bottleneck(256, 64),
                        testmodels.Bottleneck(256, 64)).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.rand(n, generator=g) - 0.5)
                m.running_var.copy_(0.5 + 1.5 * torch.rand(n, generator=g))
                m.weight.copy_(0.5 + torch.rand(n, generator=g))
                m.bias.copy_(0.4 * torch.rand(n, generator=g) - 0.2)
    return net


def _kinds(gm):
    return [type(m).__name__ for m in gm.modules()]


def test_fuse_structure_unchanged_and_no_pending_leak_on_cpu():
    """CPU: the rewrite produces the module types and the fusion count it always did, and no pending
    object leaves a module: the optimized CPU model returns the unfused model's output, and a
    deferring conv called on CPU tensors (fp32 and bf16) returns a plain tensor."""
    from wam_amd import model_fuse
    net = _stage2_stack()
    gm, n = model_fuse.fuse_elementwise(optimize_for_input_grad(net, fuse=False))
    kinds = _kinds(gm)
    assert n == 9
    assert kinds.count("ConvBiasReLU") == 6 and kinds.count("AddBiasReLU") == 3 and kinds.count("ConvNoBias") == 4
    assert sum(getattr(m, "link_in", None) is not None for m in gm.modules()) == 2
    assert sum(getattr(m, "link_out", None) is not None for m in gm.modules()) == 2
    assert sum(bool(getattr(m, "defer", False)) for m in gm.modules()) == 3
    assert sum(getattr(m, "link_src", None) is not None for m in gm.modules()) == 2
    # the rewrite is not applied to a CPU model (the fused conv -> ReLU ops have no CPU path), so
    # the optimized CPU model is the unfused graph and returns the unfused model's output
    x = torch.randn(2, 64, 8, 8)
    cpu = optimize_for_input_grad(net)
    assert "ConvNoBias" not in _kinds(cpu)
    assert torch.equal(cpu(x), optimize_for_input_grad(net, fuse=False)(x))
    # the tail modules themselves on CPU tensors: a deferring conv returns a plain tensor (fp32, and
    # bf16 channels_last, where its weight is `pointwise`), and the add takes the torch path
    for dtype in (torch.float32, torch.bfloat16):
        g16 = gm.to(dtype)
        for name, conv in g16.named_modules():
            if not getattr(conv, "defer", False):
                continue
            k = conv.weight.shape[1]
            xin = torch.randn(2, k, 5, 5).to(dtype).contiguous(memory_format=torch.channels_last)
            a = conv(xin)
            assert isinstance(a, torch.Tensor) and a.dtype == dtype
            assert torch.equal(a, nn.functional.conv2d(xin, conv.weight))
            tail = model_fuse.AddBiasReLU(torch.randn(a.shape[1]).to(dtype), None)
            s = torch.randn_like(a)
            assert torch.equal(tail(a, s), torch.relu(a + tail.bias_a.view(1, -1, 1, 1) + s))
    r50 = model_fuse.fuse_elementwise(optimize_for_input_grad(testmodels.resnet50(seed=0), fuse=False))
    assert r50[1] == 1 + 16 * 2 + 16 + 1
    assert sum(bool(getattr(m, "defer", False)) for m in r50[0].modules()) == 16


@pytest.mark.gpu
def test_gpu_stage2_stack_fused_tail_matches_float64(monkeypatch):
    """Stage-2 bottleneck stack in bf16 channels_last at 2 x 64 x 56 x 56: output and input gradient
    against the float64 CPU model by the rule of test_gpu_fused_model_matches_unfused (fused error
    <= 2 x unfused error + the 1e-2 bf16 floor), the fused launches counted, and two forwards
    followed by their two backwards in reverse order (skip-linked blocks included)."""
    L = _lib()
    net = _stage2_stack()
    torch.manual_seed(2)
    x = torch.randn(2, 64, 56, 56)
    x64 = x.double().requires_grad_(True)
    o64 = net.double()(x64)
    (g64,) = torch.autograd.grad(o64[:, 7].sum(), x64)
    net = net.float().cuda()
    fmt = torch.channels_last
    ref = optimize_for_input_grad(net, dtype=torch.bfloat16, fuse=False).to(memory_format=fmt)
    fus = optimize_for_input_grad(net, dtype=torch.bfloat16, fuse=True).to(memory_format=fmt)
    xd = x.cuda().bfloat16().contiguous(memory_format=fmt)

    calls = []
    real = L.lib.wam_pw_gemm

    def counted(mode, *a):
        assert int(mode) & ROUNDED  # the model's launches keep the two-kernel path's rounding
        calls.append(int(mode) & 1)
        return real(mode, *a)

    monkeypatch.setattr(L.lib, "wam_pw_gemm", counted)
    errs = []
    for m in (ref, fus):
        del calls[:]
        xx = xd.detach().requires_grad_(True)
        o = m(xx)
        assert isinstance(o, torch.Tensor)
        (g,) = torch.autograd.grad(o[:, 7].float().sum(), xx)
        oe = ((o.double().cpu() - o64.detach()).abs().max() / o64.abs().max()).item()
        d = (g.double().cpu() - g64).flatten(1).norm(dim=1) / g64.flatten(1).norm(dim=1)
        errs.append((oe, d.median().item(), d.max().item()))
        launched = list(calls)
    (oe_r, ge_r, _), (oe_f, ge_f, gmax_f) = errs
    print("stage-2 stack errors (unfused, fused):", errs, "launches:", launched)
    assert launched.count(TAIL) == 3, launched  # one fused tail per block
    assert launched.count(MASK) == 2, launched  # conv1's input gradient + producer mask, blocks 2 and 3
    assert oe_f <= 2 * oe_r + 1e-2, errs
    assert ge_f <= 2 * ge_r + 1e-2, errs
    assert gmax_f <= 0.5, errs

    # the fused launches round the GEMM result as the two-kernel path does, so the model computes
    # what it computes with the routes switched off: equal wherever the two fp32 accumulation orders
    # round to the same bf16 value (an accumulation error of ~1e-6 against a bf16 spacing of ~4e-3:
    # a few elements in 10^4 per layer at most), hence far inside the 1e-2 bf16 floor used above
    from wam_amd import model_fuse
    xx = xd.detach().requires_grad_(True)
    o_f = fus(xx)
    (g_f,) = torch.autograd.grad(o_f[:, 7].float().sum(), xx)
    monkeypatch.setattr(model_fuse, "_PW_ROUTES", set())
    del calls[:]
    xx = xd.detach().requires_grad_(True)
    o_p = fus(xx)
    (g_p,) = torch.autograd.grad(o_p[:, 7].float().sum(), xx)
    assert not calls  # the two-kernel path
    monkeypatch.undo()
    monkeypatch.setattr(L.lib, "wam_pw_gemm", counted)
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()  # noqa: E731
    print("fused vs two-kernel path: output rel L2 %.3e (%d of %d elements differ), gradient rel L2 %.3e" % (
        rel(o_f, o_p), int((o_f != o_p).sum()), o_f.numel(), rel(g_f, g_p)))
    assert rel(o_f, o_p) <= 1e-2 and rel(g_f, g_p) <= 5e-2

    # two forwards, then their backwards in reverse order: the skip-gradient boxes stay per call
    xs = [xd, torch.randn_like(xd)]

    def fwd(v):
        xx = v.detach().requires_grad_(True)
        return xx, fus(xx)[:, 3].float().sum()

    pairs = []
    for v in xs:
        xx, loss = fwd(v)
        pairs.append(torch.autograd.grad(loss, xx)[0].float())
    (x0, l0), (x1, l1) = fwd(xs[0]), fwd(xs[1])
    g1 = torch.autograd.grad(l1, x1)[0].float()
    g0 = torch.autograd.grad(l0, x0)[0].float()

    def close(a, b):
        d = (a - b).flatten(1).norm(dim=1) / b.flatten(1).norm(dim=1)
        return bool((d < 5e-2).all())
    assert close(g0, pairs[0]) and close(g1, pairs[1])
