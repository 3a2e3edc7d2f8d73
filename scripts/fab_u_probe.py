#!/usr/bin/env python3
"""What an untargeted FAB iteration costs: one forward with autograd, K backward passes off its retained graph
with one ee_fab_diff_f32 and one ee_fab_select_f32 each, the projection, the step, one eval forward and the commit.

Eval mode, batch 100 of synthetic 3x64x64 images, K = 200 classes, on `resnet18` (the Tiny-ImageNet model; untrained, labels are its own
clean predictions).  The iteration: the captured graph of engine.fab_u_loop (one iteration per graph), CUDA events around one replay,
median of `reps`.  Beside it, as scripts/fab_probe.py measures them: a PGD iteration ((t100 - t20) / 80 of whole graph-replayed runs), an
eval forward (a captured graph of 16, per forward) and a FAB-T iteration towards one target.  The select launch alone: CUDA events around
50 launches on a gradient of a real run, per launch, with and without the copy (first = 1 on a fresh state always improves; a second
launch of the same class never does).

    python scripts/fab_u_probe.py [reps] [--norm Linf|L2|L1]   -> one text line, then one JSON line
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
        raise SystemExit("fab_u_probe: needs a ROCm device (a time taken on the host says nothing)")
    argv = sys.argv[1:]
    norm = "Linf"
    if "--norm" in argv:
        k = argv.index("--norm")
        if k + 1 >= len(argv) or argv[k + 1] not in ops.FAB_METRICS:
            raise SystemExit("fab_u_probe: --norm takes one of %s" % sorted(ops.FAB_METRICS))
        norm = argv[k + 1]
        del argv[k:k + 2]
    reps = int(argv[0]) if argv else 7
    dev = torch.device("cuda", 0)
    eps = {"Linf": 16 / 255, "L2": 0.5, "L1": 12.0}[norm]

    class Args:
        random, epsilon = True, 16 / 255

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def median(v):
        return sorted(v)[len(v) // 2]

    torch.manual_seed(0)
    m = M.make_resnet(18, "tiny").to(dev).eval()
    x = torch.rand(100, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        order = ops.topk(m(x).float().contiguous(), None, 2)[0]
    y, t = order[:, 0].contiguous(), order[:, 1].contiguous()
    K = 200
    out = {"model": "resnet18", "batch": 100, "K": K, "norm": norm, "reps": reps}

    # the shared work, as scripts/fab_probe.py takes it
    runs = {"pgd": lambda k: A.PGD(m, Args, x, y, k, 2 / 255), "fab_t": lambda k: engine.fab_loop(m, x, y, t, k, 16 / 255)}
    for fn in runs.values():
        for k in (100, 20, 100, 20):
            fn(k)
    torch.cuda.synchronize()
    ms = {(n, k): [] for n in runs for k in (100, 20)}
    for _ in range(reps):
        for k in (100, 20):
            for n, fn in runs.items():
                ms[(n, k)].append(timed(lambda: fn(k)))
    for n in runs:
        out[n + "_iter_ms"] = round((median(ms[(n, 100)]) - median(ms[(n, 20)])) / 80, 4)
    xs = x.clone()

    def forward(model):
        with torch.no_grad():
            model(xs)

    graph = engine._Captured(m, dev, 16).capture(m, engine._times(16, forward), warmup=forward).graph
    graph.replay()
    torch.cuda.synchronize()
    out["eval_fwd_ms"] = round(median([timed(graph.replay) for _ in range(reps)]) / 16, 4)

    # the untargeted iteration: one replay of its one-iteration graph
    loop = (lambda n: engine.fab_u_l1_loop(m, x, y, n, eps, nclass=K)) if norm == "L1" else \
        (lambda n: engine.fab_u_loop(m, x, y, n, eps, norm=norm, nclass=K))
    res = loop(2)  # captures, then two replays
    gs = next(v for k, v in engine._GRAPHS.items() if k[0] in ("fab_u", "fab_u_l1"))
    gs.run.start(m)
    gs.graph.replay()
    torch.cuda.synchronize()
    out["fab_u_iter_ms"] = round(median([timed(gs.graph.replay) for _ in range(reps)]), 3)
    out["fab_u_non_robust_after_2"] = round(1.0 - float(res[1].float().mean()), 3)

    # the select launch alone
    run = gs.run
    g = run.w.clone()
    z = torch.randn(100, K, device=dev)
    st = (torch.empty(100, device=dev), torch.empty(100, dtype=torch.int32, device=dev), torch.empty_like(g), torch.empty(100, device=dev))
    yk = torch.zeros(100, dtype=torch.int64, device=dev)
    for name, first in (("copy", 1), ("nocopy", 0)):
        ops.fab_select(g, z, yk, 1, norm, *st, first=1)
        launch = lambda: [ops.fab_select(g, z, yk, 1, norm, *st, first=first) for _ in range(50)]
        launch()
        torch.cuda.synchronize()
        out["select_%s_us" % name] = round(1e3 * median([timed(launch) for _ in range(reps)]) / 50, 2)

    bwd = out["pgd_iter_ms"] - out["eval_fwd_ms"]
    out["fab_u_over_fab_t"] = round(out["fab_u_iter_ms"] / out["fab_t_iter_ms"], 2)
    out["per_class_ms"] = round((out["fab_u_iter_ms"] - out["fab_t_iter_ms"]) / (K - 1), 4)
    print("resnet18, K = %d, %s: untargeted FAB %.3f ms/iter = x%.2f of a FAB-T iteration (%.4f ms); PGD %.4f ms/iter, eval forward %.4f ms "
          "(PGD - forward = %.4f ms); per extra class %.4f ms; select launch %.1f us with the copy, %.1f us without"
          % (K, norm, out["fab_u_iter_ms"], out["fab_u_over_fab_t"], out["fab_t_iter_ms"], out["pgd_iter_ms"], out["eval_fwd_ms"], bwd,
             out["per_class_ms"], out["select_copy_us"], out["select_nocopy_us"]), flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
