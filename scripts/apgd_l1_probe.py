#!/usr/bin/env python3
"""What one APGD-CE iteration in the L1 threat model costs next to one Linf iteration of the same build, and what its launches cost alone:
ee_apgd_step_l1_f32 (resident and streaming), ee_l1_proj_f32 and ee_apgd_book_l1_f32 (at a checkpoint: with the nonzero count) next to
ee_apgd_step_f32 and ee_apgd_step_l2_f32.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, graph replay (EEADV_GRAPH=1), on `resnet18` and `resnet18_EE_square` (the
Tiny-ImageNet models); eps = 16/255 for Linf, 12 for L1, 0.5 for the L2 step.  Per-iteration time: CUDA events around whole attacks of 100
and of 20 iterations, alternating windows of the two norms, median of `reps`, (t100 - t20) / 80 - the difference leaves out what an attack
pays once (for L1: the start's projection).  The launches alone: 100 consecutive launches of one kernel on the run's own buffers captured
into a graph, events around its replay, median of `reps`, divided by 100 (the buffers stay in L2 / MALL between launches, as they do
between the select and the step of a real iteration).  The L1 step runs with the ball active in every launch: each one steps out of the
ball by step = eps and projects back.  The networks are untrained: labels are their own clean predictions.

    python scripts/apgd_l1_probe.py [reps]      -> a text line, then one JSON line per model, then one for the launches alone
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
        raise SystemExit("apgd_l1_probe: needs a ROCm device (a time taken on the host says nothing)")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    dev = torch.device("cuda", 0)
    eps_inf, eps_1, eps_2 = 16 / 255, 12.0, 0.5

    class ArgsInf:
        random, epsilon = True, eps_inf

    class Args1:
        random, epsilon = True, eps_1

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
        l1 = lambda k: A.APGD_L1(m, Args1, x, y, k, "ce")  # noqa: E731
        for k in (100, 20, 100, 20):  # captures and warm-up
            linf(k)
            l1(k)
        torch.cuda.synchronize()
        ms = {key: [] for key in (("l1", 100), ("l1", 20), ("linf", 100), ("linf", 20))}
        for _ in range(reps):
            for (n, k), fn in ((("l1", 100), l1), (("linf", 100), linf), (("l1", 20), l1), (("linf", 20), linf)):
                ms[(n, k)].append(timed(lambda: fn(k)))
        out = {"model": name, "batch": 100, "reps": reps}
        for n in ("l1", "linf"):
            out[n + "_iter_ms"] = round((median(ms[(n, 100)]) - median(ms[(n, 20)])) / 80, 4)
            out[n + "_iter_ms_spread"] = [round((a - b) / 80, 4) for a, b in zip(sorted(ms[(n, 100)]), sorted(ms[(n, 20)]))][::max(reps - 1, 1)]
        out["l1_over_linf"] = round(out["l1_iter_ms"] / out["linf_iter_ms"], 4)
        out["l1_minus_linf_us"] = round(1e3 * (out["l1_iter_ms"] - out["linf_iter_ms"]), 1)
        print("%s: L1 iteration %.4f ms, Linf iteration %.4f ms (x%.4f, %+.1f us)" % (name, out["l1_iter_ms"], out["linf_iter_ms"],
              out["l1_over_linf"], out["l1_minus_linf_us"]), flush=True)
        print(json.dumps(out), flush=True)
        engine.clear_graphs()

    # the launches alone, on buffers of the run's shape
    B, n_launch = 100, 100
    g = torch.Generator().manual_seed(2)
    x0 = torch.rand(B, 3, 64, 64, generator=g).to(dev)
    grad = torch.randn(B, 3, 64, 64, generator=g).to(dev)
    u = (x0 + torch.randn(B, 3, 64, 64, generator=g).to(dev)).contiguous()
    x, x_old, x1, z = x0.clone(), x0.clone(), x0.clone(), x0.clone()
    step2 = torch.full((B,), 2 * eps_2, device=dev)
    step1 = torch.full((B,), eps_1, device=dev)
    topk = torch.full((B,), 0.2, device=dev)
    counter = torch.ones(1, dtype=torch.int32, device=dev)
    norms = torch.zeros(3, B, device=dev)
    scal = torch.zeros(ops.L1_SCAL_ROWS, B, device=dev)
    loss, pred = torch.zeros(B, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
    fstate, istate = torch.ones(4, B, device=dev), torch.ones(4, B, dtype=torch.int32, device=dev)
    spstate = torch.full((2, B), 3 * 64 * 64, dtype=torch.int32, device=dev)
    sched = torch.full((4,), 2, dtype=torch.int32, device=dev)  # every iteration closes a checkpoint: the count runs
    launches = {
        "ee_apgd_step_f32": lambda: ops.apgd_step_(x, x_old, grad, x0, step2, counter, eps_inf),
        "ee_apgd_step_l2_f32 resident": lambda: ops.apgd_step_l2_(x, x_old, grad, x0, step2, counter, eps_2, norms, "resident"),
        "ee_apgd_step_l1_f32 resident": lambda: ops.apgd_step_l1_(x1, grad, x0, step1, topk, eps_1, scal, "resident"),
        "ee_apgd_step_l1_f32 streaming": lambda: ops.apgd_step_l1_(x1, grad, x0, step1, topk, eps_1, scal, "streaming"),
        "ee_l1_proj_f32 resident": lambda: ops.l1_proj(u, x0, eps_1, out=z, scal=scal, path="resident"),
        "ee_apgd_book_l1_f32 checkpoint": lambda: ops.apgd_book_l1_(loss, pred, x1, z, x0, fstate, istate, topk, spstate, counter, sched, eps_1),
    }
    out = {"launch": "alone", "batch": B, "per_sample": 3 * 64 * 64, "launches_per_graph": n_launch, "reps": reps}
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
        if name.startswith("ee_apgd_step_l1"):
            out[name + " active samples"] = int((scal[ops.L1_S_LAMBDA] > 0).sum().item())
    print("launch alone: " + ", ".join("%s %.2f us" % (k, out[k + " us"]) for k in launches), flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
