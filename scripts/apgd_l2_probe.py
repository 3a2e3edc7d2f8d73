#!/usr/bin/env python3
"""What one APGD-CE iteration in the L2 threat model costs next to one Linf iteration of the same build, and what the step launch costs
alone: ee_apgd_step_l2_f32 (resident and streaming) next to ee_apgd_step_f32.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, graph replay (EEADV_GRAPH=1), on `resnet18` and `resnet18_EE_square` (the
Tiny-ImageNet models); eps = 16/255 for Linf, 0.5 for L2.  Per-iteration time: CUDA events around whole attacks of 100 and of 20 iterations,
alternating windows of the two norms, median of `reps`, (t100 - t20) / 80 - the difference leaves out what an attack pays once.  The step
launches: 100 consecutive launches of one kernel on the run's own buffers captured into a graph, events around its replay, median of
`reps`, divided by 100 (the buffers stay in L2 / MALL between launches, as they do between the select and the step of a real iteration).
The networks are untrained: labels are their own clean predictions.

    python scripts/apgd_l2_probe.py [reps]      -> a text line, then one JSON line per model, then one for the step launches
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


def main():
    os.environ["EEADV_GRAPH"] = "1"
    sys.path[:0] = [PKG]
    import torch
    import utils.attacks as A
    from eeadv import engine, models as M, ops

    if not torch.cuda.is_available():
        raise SystemExit("apgd_l2_probe: needs a ROCm device (a time taken on the host says nothing)")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    dev = torch.device("cuda", 0)
    eps_inf, eps_2 = 16 / 255, 0.5

    class ArgsInf:
        random, epsilon = True, eps_inf

    class Args2:
        random, epsilon = True, eps_2

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def median(v):
        return sorted(v)[len(v) // 2]

    for name in ("resnet18", "resnet18_EE_square"):
        torch.manual_seed(0)
        if name == "resnet18":
            m = M.make_resnet(18, "tiny")
        else:
            m = M.make_resnet_ee(18, "tiny", True, cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                                 type_canny="CannyFilter_step125_1", epsilon=eps_inf, n_queries=1)
        m = m.to(dev).eval()
        g = torch.Generator().manual_seed(1)
        x = torch.rand(100, 3, 64, 64, generator=g).to(dev)
        with torch.no_grad():
            y = m(x).argmax(1)
        linf = lambda k: A.APGD(m, ArgsInf, x, y, k, "ce")  # noqa: E731
        l2 = lambda k: A.APGD(m, Args2, x, y, k, "ce", norm="L2")  # noqa: E731
        for k in (100, 20, 100, 20):  # captures and warm-up
            linf(k)
            l2(k)
        torch.cuda.synchronize()
        ms = {key: [] for key in (("l2", 100), ("l2", 20), ("linf", 100), ("linf", 20))}
        for _ in range(reps):
            for (n, k), fn in ((("l2", 100), l2), (("linf", 100), linf), (("l2", 20), l2), (("linf", 20), linf)):
                ms[(n, k)].append(timed(lambda: fn(k)))
        out = {"model": name, "batch": 100, "reps": reps}
        for n in ("l2", "linf"):
            out[n + "_iter_ms"] = round((median(ms[(n, 100)]) - median(ms[(n, 20)])) / 80, 4)
            out[n + "_iter_ms_spread"] = [round((a - b) / 80, 4) for a, b in zip(sorted(ms[(n, 100)]), sorted(ms[(n, 20)]))][::max(reps - 1, 1)]
        out["l2_over_linf"] = round(out["l2_iter_ms"] / out["linf_iter_ms"], 4)
        out["l2_minus_linf_us"] = round(1e3 * (out["l2_iter_ms"] - out["linf_iter_ms"]), 1)
        print("%s: L2 iteration %.4f ms, Linf iteration %.4f ms (x%.4f, %+.1f us)" % (name, out["l2_iter_ms"], out["linf_iter_ms"],
              out["l2_over_linf"], out["l2_minus_linf_us"]), flush=True)
        print(json.dumps(out), flush=True)
        engine.clear_graphs()

    # the step launches alone, on buffers of the run's shape
    B, n_launch = 100, 100
    g = torch.Generator().manual_seed(2)
    x0 = torch.rand(B, 3, 64, 64, generator=g).to(dev)
    grad = torch.randn(B, 3, 64, 64, generator=g).to(dev)
    x, x_old = x0.clone(), x0.clone()
    step = torch.full((B,), 2 * eps_2, device=dev)
    counter = torch.ones(1, dtype=torch.int32, device=dev)
    norms = torch.zeros(3, B, device=dev)
    launches = {
        "ee_apgd_step_f32": lambda: ops.apgd_step_(x, x_old, grad, x0, step, counter, eps_inf),
        "ee_apgd_step_l2_f32 resident": lambda: ops.apgd_step_l2_(x, x_old, grad, x0, step, counter, eps_2, norms, "resident"),
        "ee_apgd_step_l2_f32 streaming": lambda: ops.apgd_step_l2_(x, x_old, grad, x0, step, counter, eps_2, norms, "streaming"),
    }
    out = {"launch": "step alone", "batch": B, "per_sample": 3 * 64 * 64, "launches_per_graph": n_launch, "reps": reps}
    for name, fn in launches.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(n_launch):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        us = [1e3 * timed(graph.replay) / n_launch for _ in range(reps)]
        out[name + " us"] = round(median(us), 2)
        out[name + " us spread"] = [round(min(us), 2), round(max(us), 2)]
    print("step launch alone: " + ", ".join("%s %.2f us" % (k, out[k + " us"]) for k in launches), flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
