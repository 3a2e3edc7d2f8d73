#!/usr/bin/env python3
"""What an L1 Square iteration costs next to the Linf and L2 Square iterations and the eval-mode forward all three are built around.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, on `resnet18` and `resnet18_EE_square` (the Tiny-ImageNet models), four
sides replayed from captured graphs of 16 iterations in the same process: (a) 16 forwards under no_grad on a static input, (b) 16 Linf
Square iterations (ee_sqatk_step_f32 -> forward -> ee_sqatk_margin_f32; eps = 16/255), (c) 16 L2 Square iterations
(ee_sqatk_step_l2_f32 in the step's place; eps = 0.5; resident), (d) 16 L1 Square iterations (ee_sqatk_step_l1_f32: commit, proposal and
the exact L1 projection in one launch; eps = 12; the resident path, and the streaming path forced on the same shape).  CUDA events
around `replays` back-to-back replays, the windows alternating (a), (b), (c), (d), (d'), median of `reps` with the spread.  Before every timed
window of an attack the run is restarted (outside the events), so its samples begin active; the share still active at the window's end
is reported, because a fooled sample costs the step launch nothing.  The networks are untrained: labels are their own clean predictions.

    python scripts/square_l1_probe.py [reps] [replays]      -> one text line and one JSON line per model
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


def main():
    sys.path[:0] = [PKG]
    import torch
    from eeadv import engine, models as M

    if not torch.cuda.is_available():
        raise SystemExit("square_l1_probe: needs a ROCm device (a time taken on the host says nothing)")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    replays = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dev = torch.device("cuda", 0)
    eps, iters, n_queries = 16 / 255, engine.MAX_ITERS_PER_GRAPH, 5000

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

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
        # (b), (c), (d), (d'): the attacks' own graphs
        runs = {}
        for key, make in (("linf", lambda: engine._SquareRun(x, y, n_queries, eps)),
                          ("l2_resident", lambda: engine._SquareRun(x, y, n_queries, 0.5, norm="L2", path="resident")),
                          ("l1_resident", lambda: engine._SquareL1Run(x, y, n_queries, 12.0, path="resident")),
                          ("l1_streaming", lambda: engine._SquareL1Run(x, y, n_queries, 12.0, path="streaming"))):
            run = make()
            run.load(x, y, 1)
            gs = engine._Captured(m, dev, iters, run).capture(m, engine._times(iters, run.iteration), start=lambda run=run: run.start(m))
            runs[key] = (run, gs.graph)
        # (a) the forward alone, captured the same way
        xs = x.clone()

        def forward(model):
            with torch.no_grad():
                model(xs)

        fg = engine._Captured(m, dev, iters).capture(m, engine._times(iters, forward)).graph

        def window(graph):
            for _ in range(replays):
                graph.replay()

        def attack(key):
            run, graph = runs[key]
            run.start(m)
            torch.cuda.synchronize()
            t = timed(lambda: window(graph)) / (iters * replays)
            return t, float((~(run.margin_min <= 0)).float().mean())

        for _ in range(2):
            window(fg)
            for key in runs:
                attack(key)
        torch.cuda.synchronize()
        t_f, t_a, active = [], {k: [] for k in runs}, {k: [] for k in runs}
        for _ in range(reps):
            t_f.append(timed(lambda: window(fg)) / (iters * replays))
            for key in runs:
                t, act = attack(key)
                t_a[key].append(t)
                active[key].append(act)
        t_f.sort()
        out = {"model": name, "batch": 100, "reps": reps, "iters_per_window": iters * replays,
               "forward_ms": round(t_f[reps // 2], 4), "forward_ms_spread": [round(t_f[0], 4), round(t_f[-1], 4)]}
        for key in runs:
            ts = sorted(t_a[key])
            out[key + "_iter_ms"] = round(ts[reps // 2], 4)
            out[key + "_iter_ms_spread"] = [round(ts[0], 4), round(ts[-1], 4)]
            out[key + "_extra_us"] = round(1e3 * (ts[reps // 2] - t_f[reps // 2]), 1)
            out[key + "_active_at_window_end"] = round(sum(active[key]) / reps, 3)
        out["l1_over_linf"] = round(out["l1_resident_iter_ms"] / out["linf_iter_ms"], 4)
        out["l1_over_l2"] = round(out["l1_resident_iter_ms"] / out["l2_resident_iter_ms"], 4)
        out["l1_minus_l2_us"] = round(1e3 * (out["l1_resident_iter_ms"] - out["l2_resident_iter_ms"]), 1)
        print("%s: eval forward %.4f ms; Square iteration Linf %.4f ms (+%.1f us), L2 %.4f ms (+%.1f us), L1 %.4f ms resident (+%.1f us), "
              "%.4f ms streaming (+%.1f us); L1 / Linf x%.3f, L1 - L2 %+.1f us; active at the window's end: Linf %.0f %%, L2 %.0f %%, L1 %.0f %%"
              % (name, out["forward_ms"], out["linf_iter_ms"], out["linf_extra_us"], out["l2_resident_iter_ms"], out["l2_resident_extra_us"],
                 out["l1_resident_iter_ms"], out["l1_resident_extra_us"], out["l1_streaming_iter_ms"], out["l1_streaming_extra_us"],
                 out["l1_over_linf"], out["l1_minus_l2_us"], 100 * out["linf_active_at_window_end"],
                 100 * out["l2_resident_active_at_window_end"], 100 * out["l1_resident_active_at_window_end"]), flush=True)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
