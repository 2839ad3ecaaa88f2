"""A/B of the fused pointwise GEMM (wam_pw_gemm) against the pair of launches it replaces, at the c2
group shapes (batch 832, bf16): M = 832 * 56^2 for (K, N) = (64, 256), M = 832 * 28^2 for (128, 512).

  tail  parent: torch.mm (ConvNoBias) + wam_ew_add_bias_relu      fused: WAM_PW_TAIL | WAM_PW_ROUNDED
  mask  parent: torch.mm (conv1's input gradient, weight untransposed) + wam_ew_relu_mask with the
        skip gradient                                              fused: WAM_PW_MASK | WAM_PW_ROUNDED with g2

HIP events around every launch (pair), `--iters` launches after warm-up; the median is reported,
with GB/s on the fused launch's algorithmic bytes (X + s|y,g2 + out + W).

usage: python scripts/kbench_pointwise.py [--iters 20] [--batch 832]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=832)
    args = ap.parse_args()
    torch.manual_seed(0)
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
