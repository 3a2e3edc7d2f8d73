#!/usr/bin/env python3
"""Records what engine.square_loop returns in Linf and in L2 on a fixed small problem, on a ROCm device:

    python tests/golden/make_square_loop_golden.py [ROOT] [OUT]

ROOT: the checkout whose package is imported (default: this one); OUT: the .npz (default tests/golden/square_loop.npz next to this file).
tests/golden/square_loop.npz was recorded on the commit before the L1 Square attack; tests/test_gpu_square_l1.py holds the same call of
the current code to it bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE, N_QUERIES, SEED = (3, 3, 9, 9), 40, 20261
RADII = {"Linf": 8 / 255, "L2": 0.5}


def problem(torch):
    """(weights [10, D], x [B,C,H,W], y [B]) on the CPU: a linear classifier, images with exact zeros and ones, one label wrong."""
    g = torch.Generator().manual_seed(5)
    D = SHAPE[1] * SHAPE[2] * SHAPE[3]
    w = torch.randn(10, D, generator=g) * 0.3
    x = torch.rand(*SHAPE, generator=g)
    x.view(-1)[::5] = 0.0
    x.view(-1)[2::5] = 1.0
    y = torch.nn.functional.linear(x.flatten(1), w).argmax(1)  # the classifier's own predictions,
    y[0] = (y[0] + 1) % 10                                     # but one sample starts misclassified
    return w, x, y


def run(torch, engine, norm, use_graph=False):
    w, x, y = problem(torch)

    class Linear(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(w.clone())

        def forward(self, v):
            return torch.nn.functional.linear(v.flatten(1), self.w)

    m = Linear().to("cuda:0").eval()
    trace = None if use_graph else []
    xa, robust, queries = engine.square_loop(m, x.to("cuda:0"), y.to("cuda:0"), N_QUERIES, RADII[norm], seed=SEED, use_graph=use_graph, trace=trace,
                                             early_exit=False, norm=norm)
    out = {norm + "_x_adv": xa.cpu().numpy(), norm + "_robust": robust.cpu().numpy(), norm + "_queries": queries.cpu().numpy()}
    if trace is not None:  # the margin of every forward: each depends on every element of its proposal
        out[norm + "_margins"] = torch.stack([t["margin"] for t in trace]).cpu().numpy()
    return out


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "square_loop.npz")
    sys.path[:0] = [os.path.join(root, "edge-enhancement_amd")]
    import torch
    from eeadv import engine
    arrays = {}
    for norm in RADII:
        arrays.update(run(torch, engine, norm))
    np.savez(out, **arrays)
    print("wrote", out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
