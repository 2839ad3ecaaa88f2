"""A/B of the fused pointwise GEMM (wam_pw_gemm) against the pair of launches it replaces, at the c2
group shapes (batch 832, bf16): M = 832 * 56^2 for (K, N) = (64, 256), M = 832 * 28^2 for (128, 512).

  tail  parent: torch.mm (ConvNoBias) + wam_ew_add_bias_relu      fused: WAM_PW_TAIL | WAM_PW_ROUNDED
  mask  parent: torch.mm (conv1's input gradient, weight untransposed) + wam_ew_relu_mask with the
        skip gradient                                              fused: WAM_PW_MASK | WAM_PW_ROUNDED with g2

HIP events around every launch (pair), `--iters` launches after warm-up; the median is reported,
with GB/s on the fused launch's algorithmic bytes (X + s|y,g2 + out + W).

--relubits times the packed-mask forms instead (wam_ew_*_bits, wam_pw_gemm | WAM_PW_BITS, the junction
sum and wam_ew_bias_maxpool_nhwc), each against the launches it replaces: see relubits().

usage: python scripts/kbench_pointwise.py [--iters 20] [--batch 832] [--relubits]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import wam_amd  # noqa: E402,F401
from wam_amd import _lib  # noqa: E402

ROUNDED = 16  # WAM_PW_ROUNDED: the form the model launches (GEMM result rounded to bf16 before the epilogue)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2] * 1e3, t[0] * 1e3  # median, min in us


def relubits(args):
    """The packed-mask forms, the junction sum and the stem pool against the launches they replace, at
    the c2 activation sizes: [832 * 56^2, 256] (block outputs of stage 2), [832 * 56^2, 64] (its conv2
    outputs) and the stem's [832, 112, 112, 64] convolution output."""
    bf = torch.bfloat16
    st = lambda: _lib.stream_of(torch.device("cuda"))  # noqa: E731
    p, L, ck = _lib.ptr, _lib.lib, _lib.check
    print("%-22s %12s | %9s | %9s %9s | %s" % ("form", "elements", "today us", "new us", "min us", "new / today"))

    def row(name, n, today, new):
        t0, _ = timed(today, args.iters)
        t1, t1min = timed(new, args.iters)
        print("%-22s %12d | %9.1f | %9.1f %9.1f | %.3f" % (name, n, t0, t1, t1min, t1 / t0), flush=True)

    for C in (256, 64):
        n = args.batch * 56 * 56 * C
        g1, g2 = torch.randn(n, device="cuda").to(bf), torch.randn(n, device="cuda").to(bf)
        a, s = torch.randn(n, device="cuda").to(bf), torch.randn(n, device="cuda").to(bf)
        b = torch.randn(C, device="cuda").to(bf)
        y = torch.relu(torch.randn(n, device="cuda")).to(bf)
        out, tmp = torch.empty_like(y), torch.empty_like(y)
        m = torch.empty(n // 8, dtype=torch.uint8, device="cuda")
        ck(L.wam_ew_add_bias_relu_bits(1, n, C, 1, p(a), p(b), p(s), p(b), p(y), p(m), st()))
        row("mask C=%d" % C, n, lambda: ck(L.wam_ew_relu_mask(1, n, p(g1), None, p(y), p(out), st())),
            lambda: ck(L.wam_ew_relu_mask_bits(1, n, p(g1), None, p(m), p(out), st())))
        row("mask + g2 C=%d" % C, n, lambda: ck(L.wam_ew_relu_mask(1, n, p(g1), p(g2), p(y), p(out), st())),
            lambda: ck(L.wam_ew_relu_mask_bits(1, n, p(g1), p(g2), p(m), p(out), st())))
        row("junction C=%d" % C, n,
            lambda: (torch.add(g1, g2, out=tmp), ck(L.wam_ew_relu_mask(1, n, p(tmp), None, p(y), p(out), st()))),
            lambda: ck(L.wam_ew_relu_mask_bits(1, n, p(g1), p(g2), p(m), p(out), st())))
        row("junction, y C=%d" % C, n,
            lambda: (torch.add(g1, g2, out=tmp), ck(L.wam_ew_relu_mask(1, n, p(tmp), None, p(y), p(out), st()))),
            lambda: ck(L.wam_ew_relu_mask(1, n, p(g1), p(g2), p(y), p(out), st())))
        row("add_bias_relu+bits C=%d" % C, n,
            lambda: ck(L.wam_ew_add_bias_relu(1, n, C, 1, p(a), p(b), p(s), p(b), p(out), st())),
            lambda: ck(L.wam_ew_add_bias_relu_bits(1, n, C, 1, p(a), p(b), p(s), p(b), p(out), p(m), st())))
        row("bias_act+bits C=%d" % C, n, lambda: ck(L.wam_ew_bias_act(1, n, C, 1, p(tmp), p(b), 1, st())),
            lambda: ck(L.wam_ew_bias_act_bits(1, n, C, 1, p(tmp), p(b), p(m), st())))
        del g1, g2, a, s, y, out, tmp, m
    # wam_pw_gemm with the packed mask: TAIL writing it, MASK (with g2, as the model launches it) reading it
    BITS = 32
    for K, N, hw in ((64, 256, 56), (128, 512, 28)):
        M = args.batch * hw * hw
        x = torch.randn(M, K, device="cuda").to(bf)
        w = (torch.randn(N, K, device="cuda") / K ** 0.5).to(bf)
        ba, bs = torch.randn(N, device="cuda").to(bf), torch.randn(N, device="cuda").to(bf)
        s = torch.randn(M, N, device="cuda").to(bf)
        y = torch.relu(torch.randn(M, N, device="cuda")).to(bf)
        out = torch.empty(M, N, device="cuda", dtype=bf)
        m = torch.empty(M * N // 8, dtype=torch.uint8, device="cuda")
        row("pw tail+bits %dx%d" % (K, N), M * N,
            lambda: ck(L.wam_pw_gemm(0 | ROUNDED, 1, M, K, N, p(x), p(w), p(ba), p(bs), p(s), None, p(out), st())),
            lambda: ck(L.wam_pw_gemm(0 | ROUNDED | BITS, 1, M, K, N, p(x), p(w), p(ba), p(bs), p(s), p(m), p(out), st())))
        ck(L.wam_ew_add_bias_relu_bits(1, M * N, N, 1, p(s), None, p(s), None, p(y), p(m), st()))
        row("pw mask, bits %dx%d" % (K, N), M * N,
            lambda: ck(L.wam_pw_gemm(1 | ROUNDED, 1, M, K, N, p(x), p(w), None, None, p(s), p(y), p(out), st())),
            lambda: ck(L.wam_pw_gemm(1 | ROUNDED | BITS, 1, M, K, N, p(x), p(w), None, None, p(s), p(m), p(out), st())))
        del x, s, y, out, m
    N, H, C = args.batch, 112, 64
    x = torch.randn(N * H * H * C, device="cuda").to(bf)
    t = x.clone()
    b = torch.randn(C, device="cuda").to(bf)
    yo = torch.empty(N * 56 * 56 * C, device="cuda", dtype=bf)
    idx = torch.empty(N * 56 * 56 * C, device="cuda", dtype=torch.uint8)
    row("stem bias+relu+pool", x.numel(),
        lambda: (ck(L.wam_ew_bias_act(1, t.numel(), C, 1, p(t), p(b), 1, st())),
                 ck(L.wam_ew_maxpool_nhwc(1, N, H, H, C, 3, 2, 1, p(t), p(yo), p(idx), st()))),
        lambda: ck(L.wam_ew_bias_maxpool_nhwc(1, N, H, H, C, 3, 2, 1, p(x), p(b), p(yo), p(idx), st())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=832)
    ap.add_argument("--relubits", action="store_true", help="the packed-mask, junction and stem-pool pairs only")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.relubits:
        return relubits(args)
    bf = torch.bfloat16
    st = lambda: _lib.stream_of(torch.device("cuda"))  # noqa: E731
    print("%-5s %-9s %10s | %9s %9s %9s | %9s %9s %7s | %s" % ("mode", "K x N", "M", "mm us", "ew us", "pair us",
                                                              "fused us", "min us", "GB/s", "fused / pair"))
    for K, N, hw in ((64, 256, 56), (128, 512, 28)):
        M = args.batch * hw * hw
        x = torch.randn(M, K, device="cuda").to(bf)
        w = (torch.randn(N, K, device="cuda") / K ** 0.5).to(bf)
        wt = w.t().contiguous()  # [K, N]: conv1's weight as stored, for the input-gradient mm
        ba, bs = torch.randn(N, device="cuda").to(bf), torch.randn(N, device="cuda").to(bf)
        s = torch.randn(M, N, device="cuda").to(bf)
        y = torch.relu(torch.randn(M, N, device="cuda")).to(bf)
        a = torch.empty(M, N, device="cuda", dtype=bf)
        out = torch.empty(M, N, device="cuda", dtype=bf)
        p = _lib.ptr
        for mode in ("tail", "mask"):
            if mode == "tail":
                mm = lambda: torch.mm(x, w.t(), out=a)  # noqa: E731
                ew = lambda: _lib.check(_lib.lib.wam_ew_add_bias_relu(1, M * N, N, 1, p(a), p(ba), p(s), p(bs),  # noqa: E731
                                                                      p(out), st()))
                fused = lambda: _lib.check(_lib.lib.wam_pw_gemm(0 | ROUNDED, 1, M, K, N, p(x), p(w), p(ba), p(bs), p(s), None,  # noqa: E731
                                                                p(out), st()))
                nbytes = 2.0 * (M * K + 2 * M * N + N * K)
            else:
                mm = lambda: torch.mm(x, wt, out=a)  # noqa: E731
                ew = lambda: _lib.check(_lib.lib.wam_ew_relu_mask(1, M * N, p(a), p(s), p(y), p(out), st()))  # noqa: E731
                fused = lambda: _lib.check(_lib.lib.wam_pw_gemm(1 | ROUNDED, 1, M, K, N, p(x), p(w), None, None, p(s), p(y),  # noqa: E731
                                                                p(out), st()))
                nbytes = 2.0 * (M * K + 3 * M * N + N * K)
            t_mm, _ = timed(mm, args.iters)
            t_ew, _ = timed(ew, args.iters)
            t_pair, _ = timed(lambda: (mm(), ew()), args.iters)
            t_f, t_fmin = timed(fused, args.iters)
            print("%-5s %-9s %10d | %9.1f %9.1f %9.1f | %9.1f %9.1f %7.0f | %.3f" % (
                mode, "%dx%d" % (K, N), M, t_mm, t_ew, t_pair, t_f, t_fmin, nbytes / t_f / 1e3, t_f / t_pair),
                flush=True)
        del x, s, y, a, out


if __name__ == "__main__":
    main()
