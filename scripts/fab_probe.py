#!/usr/bin/env python3
"""What a FAB-T iteration costs next to the work it shares with the attacks that exist: one PGD iteration (forward + backward) plus one
eval forward.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, graph replay (EEADV_GRAPH=1), on `resnet18` and `resnet18_EE_square`
(the Tiny-ImageNet models).  Per-iteration time: CUDA events around whole runs of 100 and of 20 iterations, alternating PGD and FAB-T
(one target: the second class of the clean logits), median of `reps`; (t100 - t20) / 80 leaves out what a run pays once.  The eval
forward: a captured graph of 16 forwards under no_grad, per forward.  The projection launch alone (2 x 100 problems of 12288 coordinates,
on a gradient and an iterate taken from a real run): CUDA events around 50 launches, per launch, on both paths.  The networks are
untrained: labels are their own clean predictions.

--norm L2 times the L2 iteration (engine.fab_loop(norm="L2"), eps = 0.5) and the L2 projection launch beside the Linf ones, in the same
run, the three attacks alternating.  --norm L1 times the L1 iteration (engine.fab_l1_loop, eps = 12) and the L1 projection launch beside
the Linf and the L2 ones, in the same run, the four attacks alternating.

--restarts adds, on `resnet18`, a FAB-T run of 2 restarts beside the others - its time per iteration is
(t100 - t20) / 160, the same graph replayed twice as often - and the start launch of a restart alone (100 rows of 12288 elements, the
kernel's own uniform draw, res = +inf), per launch, on both paths.

    python scripts/fab_probe.py [reps] [--norm Linf|L2|L1] [--restarts]   -> a few text lines, then one JSON line per model
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
        raise SystemExit("fab_probe: needs a ROCm device (a time taken on the host says nothing)")
    argv = sys.argv[1:]
    norm = "Linf"
    if "--norm" in argv:
        k = argv.index("--norm")
        if k + 1 >= len(argv) or argv[k + 1] not in engine.FAB_NORMS + ("L1",):
            raise SystemExit("fab_probe: --norm takes one of %s" % (list(engine.FAB_NORMS) + ["L1"],))
        norm = argv[k + 1]
        del argv[k:k + 2]
    restarts = "--restarts" in argv
    if restarts:
        argv.remove("--restarts")
    l1 = norm == "L1"
    l2 = norm == "L2" or l1  # the L1 run is measured beside both
    reps = int(argv[0]) if argv else 7
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

    for name in ("resnet18",) if restarts else ("resnet18", "resnet18_EE_square"):
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
            order = ops.topk(m(x).float().contiguous(), None, 2)[0]
        y, t = order[:, 0].contiguous(), order[:, 1].contiguous()
        runs = {"pgd": lambda k: A.PGD(m, Args, x, y, k, 2 / 255), "fab_t": lambda k: engine.fab_loop(m, x, y, t, k, eps)}
        if l2:
            runs["fab_t_l2"] = lambda k: engine.fab_loop(m, x, y, t, k, 0.5, norm="L2")
        if l1:
            runs["fab_t_l1"] = lambda k: engine.fab_l1_loop(m, x, y, t, k, 12.0)
        r2 = restarts and name == "resnet18"
        if r2:
            runs["fab_t_r2"] = lambda k: engine.fab_loop(m, x, y, t, k, eps, n_restarts=2, seed=1)
        for fn in runs.values():  # captures and warm-up of both lengths
            for k in (100, 20, 100, 20):
                fn(k)
        torch.cuda.synchronize()
        ms = {(n, k): [] for n in runs for k in (100, 20)}
        for _ in range(reps):
            for k in (100, 20):
                for n, fn in runs.items():
                    ms[(n, k)].append(timed(lambda: fn(k)))
        out = {"model": name, "batch": 100, "reps": reps}
        for n in runs:
            t100, t20 = median(ms[(n, 100)]), median(ms[(n, 20)])
            out[n + "_ms_100"], out[n + "_ms_20"] = round(t100, 3), round(t20, 3)
            out[n + "_iter_ms"] = round((t100 - t20) / (160 if n == "fab_t_r2" else 80), 4)
        # the eval forward, replayed from a graph of 16
        xs = x.clone()

        def forward(model):
            with torch.no_grad():
                model(xs)

        graph = engine._Captured(m, dev, 16).capture(m, engine._times(16, forward), warmup=forward).graph
        graph.replay()
        torch.cuda.synchronize()
        out["eval_fwd_ms"] = round(median([timed(graph.replay) for _ in range(reps)]) / 16, 4)
        shared = out["pgd_iter_ms"] + out["eval_fwd_ms"]
        out["fab_over_shared"] = round(out["fab_t_iter_ms"] / shared, 4)
        out["fab_extra_us_per_iter"] = round(1e3 * (out["fab_t_iter_ms"] - shared), 1)
        # the projection launch alone, on the state of a real run's third iteration
        run = engine._FabRun(x, y, 3, eps)
        run.load(x, y, t)
        run.start(m)
        for _ in range(2):
            run.iteration(m)
        w = engine.input_gradient(m, run.x, run.spec).contiguous()
        xi = run.x.detach()
        for path in ("resident", "streaming"):
            launch = lambda: [ops.fab_proj_linf(xi, run.x0, w, run.df, path, run.scal) for _ in range(50)]
            launch()
            torch.cuda.synchronize()
            out["proj_%s_us" % path] = round(1e3 * median([timed(launch) for _ in range(reps)]) / 50, 2)
        res = engine.fab_loop(m, x, y, t, 100, eps)
        out["fab_t_non_robust_after_one_target"] = round(1.0 - float(res[1].float().mean()), 3)
        if l2:
            out["fab_l2_over_linf"] = round(out["fab_t_l2_iter_ms"] / out["fab_t_iter_ms"], 4)
            out["fab_l2_minus_linf_us_per_iter"] = round(1e3 * (out["fab_t_l2_iter_ms"] - out["fab_t_iter_ms"]), 1)
            run2 = engine._FabRun(x, y, 3, eps, norm="L2")  # the L2 projection launch on the state of an L2 run's third iteration
            run2.load(x, y, t)
            run2.start(m)
            for _ in range(2):
                run2.iteration(m)
            w2 = engine.input_gradient(m, run2.x, run2.spec).contiguous()
            x2 = run2.x.detach()
            for path in ("resident", "streaming"):
                launch = lambda: [ops.fab_proj_l2(x2, run2.x0, w2, run2.df, path, run2.scal) for _ in range(50)]
                launch()
                torch.cuda.synchronize()
                out["proj_l2_%s_us" % path] = round(1e3 * median([timed(launch) for _ in range(reps)]) / 50, 2)
            res = engine.fab_loop(m, x, y, t, 100, 0.5, norm="L2")
            out["fab_t_l2_non_robust_after_one_target"] = round(1.0 - float(res[1].float().mean()), 3)
        if l1:
            out["fab_l1_over_linf"] = round(out["fab_t_l1_iter_ms"] / out["fab_t_iter_ms"], 4)
            out["fab_l1_over_l2"] = round(out["fab_t_l1_iter_ms"] / out["fab_t_l2_iter_ms"], 4)
            out["fab_l1_minus_linf_us_per_iter"] = round(1e3 * (out["fab_t_l1_iter_ms"] - out["fab_t_iter_ms"]), 1)
            run1 = engine._FabL1Run(x, y, 3, 12.0)  # the L1 projection launch on the state of an L1 run's third iteration
            run1.load(x, y, t)
            run1.start(m)
            for _ in range(2):
                run1.iteration(m)
            w1 = engine.input_gradient(m, run1.x, run1.spec).contiguous()
            x1 = run1.x.detach()
            for path in ("resident", "streaming"):
                launch = lambda: [ops.fab_proj_l1(x1, run1.x0, w1, run1.df, path, run1.scal) for _ in range(50)]
                launch()
                torch.cuda.synchronize()
                out["proj_l1_%s_us" % path] = round(1e3 * median([timed(launch) for _ in range(reps)]) / 50, 2)
            res = engine.fab_l1_loop(m, x, y, t, 100, 12.0)
            out["fab_t_l1_non_robust_after_one_target"] = round(1.0 - float(res[1].float().mean()), 3)
        print("%s: PGD %.4f ms/iter + eval forward %.4f ms = %.4f ms; FAB-T %.4f ms/iter (x%.3f, +%.1f us); projection launch %.1f us resident, "
              "%.1f us streaming" % (name, out["pgd_iter_ms"], out["eval_fwd_ms"], shared, out["fab_t_iter_ms"], out["fab_over_shared"],
                                     out["fab_extra_us_per_iter"], out["proj_resident_us"], out["proj_streaming_us"]), flush=True)
        if l2:
            print("%s: L2 FAB-T %.4f ms/iter (x%.3f of the Linf iteration, %+.1f us); L2 projection launch %.1f us resident, %.1f us streaming"
                  % (name, out["fab_t_l2_iter_ms"], out["fab_l2_over_linf"], out["fab_l2_minus_linf_us_per_iter"], out["proj_l2_resident_us"],
                     out["proj_l2_streaming_us"]), flush=True)
        if l1:
            print("%s: L1 FAB-T %.4f ms/iter (x%.3f of the Linf iteration, %+.1f us; x%.3f of the L2 one); L1 projection launch %.1f us resident, "
                  "%.1f us streaming" % (name, out["fab_t_l1_iter_ms"], out["fab_l1_over_linf"], out["fab_l1_minus_linf_us_per_iter"],
                                         out["fab_l1_over_l2"], out["proj_l1_resident_us"], out["proj_l1_streaming_us"]), flush=True)
        if r2:
            xs_, res_ = torch.empty_like(x), torch.full((100,), float("inf"), device=dev)
            for path in ("resident", "streaming"):
                launch = lambda: [ops.fab_start_(xs_, x, res_, eps, "Linf", seed=1, path=path) for _ in range(50)]
                launch()
                torch.cuda.synchronize()
                out["start_%s_us" % path] = round(1e3 * median([timed(launch) for _ in range(reps)]) / 50, 2)
            out["fab_r2_over_r1_iter"] = round(out["fab_t_r2_iter_ms"] / out["fab_t_iter_ms"], 4)
            out["fab_r2_once_ms"] = round(out["fab_t_r2_ms_100"] - 200 * out["fab_t_r2_iter_ms"], 3)  # what a 2-restart run pays once
            out["fab_r1_once_ms"] = round(out["fab_t_ms_100"] - 100 * out["fab_t_iter_ms"], 3)
            print("%s: FAB-T with 2 restarts %.4f ms/iter (x%.3f of one run's %.4f); start launch %.1f us resident, %.1f us streaming; "
                  "paid once per call: %.3f ms with 2 restarts, %.3f ms with one"
                  % (name, out["fab_t_r2_iter_ms"], out["fab_r2_over_r1_iter"], out["fab_t_iter_ms"], out["start_resident_us"],
                     out["start_streaming_us"], out["fab_r2_once_ms"], out["fab_r1_once_ms"]), flush=True)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
