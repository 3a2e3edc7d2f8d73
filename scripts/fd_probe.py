#!/usr/bin/env python3
"""The feature-denoising product (ee_fd.hip, ops.fd_fwd / ops.fd_bwd) against the matmul composite in the reference's association, at batch 32
on the four ResNet-18/34 block shapes at 224 x 224 and the three Bottleneck-width shapes the kernel class takes.  Graph-replayed, un-profiled
timing (as scripts/hfs_bench.py); writes profiles/fd_probe.txt.  The share of HBM peak is taken against the minimal traffic of a pass: read
X once and write F once (forward), read X and dF once and write dX once more (forward + backward: 5 maps of 4 B per element)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "edge-enhancement_amd"))
import torch  # noqa: E402

from eeadv import ops  # noqa: E402

PEAK_GBS = 8000.0
SHAPES = [(64, 3136), (128, 784), (256, 196), (512, 49), (256, 3136), (1024, 196), (2048, 49)]


def timeit(fn, iters=20, reps=5):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / (iters * reps)


def composite_fwd(x, s):
    xt = x.transpose(1, 2)
    if x.shape[1] > x.shape[2]:
        a = torch.matmul(xt, x)
        return torch.matmul(x, a) * s, a
    a = torch.matmul(x, xt)
    return torch.matmul(a, x) * s, a


def composite_bwd(x, d, a, s):
    if x.shape[1] > x.shape[2]:
        b = torch.matmul(d.transpose(1, 2), x)
        return (torch.matmul(d, a) + torch.matmul(x, b + b.transpose(1, 2))) * s
    m = torch.matmul(d, x.transpose(1, 2))
    return (torch.matmul(m + m.transpose(1, 2), x) + torch.matmul(a, d)) * s


def main(batch=32):
    lines = ["feature-denoising product, batch %d, %s; us per call, graph-replayed; share of %.0f GB/s against the minimal traffic"
             % (batch, torch.cuda.get_device_name(0), PEAK_GBS),
             "%-14s %-8s %10s %10s %7s %10s %10s %7s %9s" % ("C x P", "form", "fwd hip", "fwd mm", "of peak", "f+b hip", "f+b mm", "of peak", "f+b mm/hip")]
    for C, P in SHAPES:
        assert ops.fd_supported(C, P)
        x, d = torch.randn(batch, C, P, device="cuda:0"), torch.randn(batch, C, P, device="cuda:0")
        s = 1.0 / P

        def both(fwd, bwd):
            f, a = fwd(x, s)
            return bwd(x, d, a, s)
        t_f, t_fm = timeit(lambda: ops.fd_fwd(x, s)), timeit(lambda: composite_fwd(x, s))
        t_b, t_bm = timeit(lambda: both(ops.fd_fwd, ops.fd_bwd)), timeit(lambda: both(composite_fwd, composite_bwd))
        nbytes = 4.0 * x.numel()
        lines.append("%-14s %-8s %10.1f %10.1f %7.3f %10.1f %10.1f %7.3f %9.2f"
                     % ("%d x %d" % (C, P), "spatial" if C > P else "channel", t_f, t_fm, 2 * nbytes / t_f / 1e3 / PEAK_GBS, t_b, t_bm,
                        5 * nbytes / t_b / 1e3 / PEAK_GBS, t_bm / t_b))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = os.environ.get("FD_PROBE_OUT", os.path.join(ROOT, "profiles", "fd_probe.txt"))
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
