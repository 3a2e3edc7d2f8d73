#!/usr/bin/env python3
"""What one EOT iteration of APGD-CE (E = 20 forward/backward pairs, one accumulate launch each, one bookkeeping / step / select) costs
next to 20 plain APGD-CE iterations - the same 20 forward/backward pairs with the bookkeeping, step and select paid 20 times.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, eps = 16/255, graph replay (EEADV_GRAPH=1), on `resnet18` and
`resnet18_EE_square` (the Tiny-ImageNet models).  Per-iteration time: CUDA events around whole attacks, alternating windows of the two,
median of `reps`: eot_iter = 20 with 6 and with 2 iterations, (t6 - t2) / 4; eot_iter = 1 with 100 and with 20 iterations, (t100 - t20) / 80 -
the differences leave out what an attack pays once (the start point and its E forward/backward pairs, the initial state).  Also: the
wall-clock time of the first eot_iter = 20 call (two warm-up executions of the 20-draw iteration, its capture, one attack), the node
count of a 20-draw iteration's graph (a capture of its own with the graph kept, hipGraphGetNodes), and what `Rand` costs per batch at
100 iterations (APGD-CE then APGD-DLR, E = 20; ONE timed call after an untimed one, not a median) next to one plain APGD-CE run.  The
networks are untrained: labels are their own clean predictions.

    python scripts/eot_probe.py [reps]      -> a text line, then one JSON line per model
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
E = 20


def _hip_runtime():
    """The HIP runtime this process already runs on (torch's copy): opened by its path, so no second instance is loaded.  The node count is
    a side figure: it leans on torch's beta raw_cuda_graph and on the first mapped libamdhip64, and any failure leaves it "unavailable"."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    return ctypes.CDLL(sorted(paths)[0]) if paths else None


def graph_nodes(torch, engine, model, x, y, eps):
    """Nodes of a captured graph of ONE iteration with E draws (a capture of its own, with the graph kept)."""
    hip = _hip_runtime()
    if hip is None or not hasattr(torch.cuda.CUDAGraph, "raw_cuda_graph"):
        return None
    run = engine._ApgdRun(x, y, 2, eps, "ce", E)
    run.load(x, x, y, None)
    run.start(model)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run.iteration(model, run.g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        run.iteration(model, run.g)
    n = ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n))
    return int(n.value) if rc == 0 else None


def main():
    os.environ["EEADV_GRAPH"] = "1"
    sys.path[:0] = [PKG]
    import torch
    import utils.attacks as A
    from eeadv import engine, models as M

    if not torch.cuda.is_available():
        raise SystemExit("eot_probe: needs a ROCm device (a time taken on the host says nothing)")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    dev = torch.device("cuda", 0)
    eps = 16 / 255

    class Args:
        random, epsilon = True, eps

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
                                 type_canny="CannyFilter_step125_1", epsilon=eps, n_queries=1)
        m = m.to(dev).eval()
        g = torch.Generator().manual_seed(1)
        x = torch.rand(100, 3, 64, 64, generator=g).to(dev)
        with torch.no_grad():
            y = m(x).argmax(1)
        plain = lambda k: A.APGD(m, Args, x, y, k, "ce")  # noqa: E731
        eot = lambda k: A.APGD(m, Args, x, y, k, "ce", eot_iter=E)  # noqa: E731
        for k in (100, 20, 100, 20):  # captures and warm-up of the yardstick
            plain(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eot(6)  # the first call: two warm-up executions, the capture, one attack
        torch.cuda.synchronize()
        first_call_s = time.perf_counter() - t0
        t6 = timed(lambda: eot(6))
        for k in (2, 6, 2):
            eot(k)
        torch.cuda.synchronize()
        ms = {key: [] for key in (("eot", 6), ("eot", 2), ("plain", 100), ("plain", 20))}
        for _ in range(reps):
            for (n, k), fn in ((("eot", 6), eot), (("plain", 100), plain), (("eot", 2), eot), (("plain", 20), plain)):
                ms[(n, k)].append(timed(lambda: fn(k)))
        out = {"model": name, "batch": 100, "reps": reps, "eot_iter": E}
        out["eot_iter_ms"] = round((median(ms[("eot", 6)]) - median(ms[("eot", 2)])) / 4, 4)
        out["plain_iter_ms"] = round((median(ms[("plain", 100)]) - median(ms[("plain", 20)])) / 80, 4)
        out["eot_iter_ms_spread"] = [round((a - b) / 4, 4) for a, b in zip(sorted(ms[("eot", 6)]), sorted(ms[("eot", 2)]))][::max(reps - 1, 1)]
        out["plain_iter_ms_spread"] = [round((a - b) / 80, 4) for a, b in zip(sorted(ms[("plain", 100)]), sorted(ms[("plain", 20)]))][::max(reps - 1, 1)]
        out["eot_over_20_plain"] = round(out["eot_iter_ms"] / (E * out["plain_iter_ms"]), 4)
        out["eot_minus_20_plain_us"] = round(1e3 * (out["eot_iter_ms"] - E * out["plain_iter_ms"]), 1)
        out["first_call_s"] = round(first_call_s, 3)
        out["capture_s"] = round(first_call_s - t6 / 1e3, 3)  # the first call less what the attack itself takes once captured
        out["iters_per_graph"] = engine._eot_chunk(6, E)
        # Rand per batch at the default budget, next to one plain APGD-CE run
        rand_ms = timed(lambda: A.APGD_Rand(m, Args, x, y, 100, E, 200))  # captures the 100-iteration E = 20 graphs of both losses
        rand_ms = timed(lambda: A.APGD_Rand(m, Args, x, y, 100, E, 200))
        out["rand_100_s"] = round(rand_ms / 1e3, 3)
        out["apgd_ce_100_ms"] = round(median(ms[("plain", 100)]), 3)
        out["rand_over_apgd_ce"] = round(rand_ms / median(ms[("plain", 100)]), 2)
        print("%s: EOT iteration (E = %d) %.3f ms, 20 plain iterations %.3f ms (x%.4f, %+.1f us); first call %.2f s, of it capture %.2f s; "
              "Rand at 100 iterations %.2f s per batch (x%.1f an APGD-CE run)" % (name, E, out["eot_iter_ms"], E * out["plain_iter_ms"],
              out["eot_over_20_plain"], out["eot_minus_20_plain_us"], out["first_call_s"], out["capture_s"], out["rand_100_s"],
              out["rand_over_apgd_ce"]), flush=True)
        print(json.dumps(out), flush=True)
        try:
            out["graph_nodes_per_iteration"] = graph_nodes(torch, engine, m, x, y, eps)
        except Exception as exc:  # noqa: BLE001 - the count is a side figure: the timings above stand without it
            out["graph_nodes_per_iteration"] = "unavailable: %s" % (exc,)
        print(json.dumps({"model": name, "graph_nodes_per_iteration": out["graph_nodes_per_iteration"]}), flush=True)
        engine.clear_graphs()


if __name__ == "__main__":
    main()
