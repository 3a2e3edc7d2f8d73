#!/usr/bin/env python3
"""What a Square-attack iteration costs next to the eval-mode forward it is built around.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, eps = 16/255, on `resnet18` and `resnet18_EE_square` (the Tiny-ImageNet
models), both sides replayed from captured graphs of 16 iterations in the same process: (a) 16 forwards under no_grad on a static input,
(b) 16 Square iterations (ee_sqatk_step_f32 -> forward -> ee_sqatk_margin_f32) over the static buffers of engine._SquareRun.  CUDA events
around `replays` back-to-back replays, alternating (a) and (b), median of `reps` with the spread.  Before every timed window of (b) the
run is restarted (outside the events), so its samples begin active; the share still active at the window's end is reported, because a
fooled sample costs the step launch nothing.  The networks are untrained: labels are their own clean predictions.

    python scripts/square_probe.py [reps] [replays]      -> one text line and one JSON line per model
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
        raise SystemExit("square_probe: needs a ROCm device (a time taken on the host says nothing)")
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
        # (b) the attack's own graph
        run = engine._SquareRun(x, y, n_queries, eps)
        run.load(x, y, 1)
        gs = engine._Captured(m, dev, iters, run).capture(m, engine._times(iters, run.iteration), start=lambda: run.start(m))
        # (a) the forward alone, captured the same way
        xs = x.clone()

        def forward(model):
            with torch.no_grad():
                model(xs)

        fg = engine._Captured(m, dev, iters).capture(m, engine._times(iters, forward)).graph

        def window(graph):
            for _ in range(replays):
                graph.replay()

        for _ in range(2):
            window(fg)
            run.start(m)
            window(gs.graph)
        torch.cuda.synchronize()
        t_f, t_s, active = [], [], []
        for _ in range(reps):
            t_f.append(timed(lambda: window(fg)) / (iters * replays))
            run.start(m)
            torch.cuda.synchronize()
            t_s.append(timed(lambda: window(gs.graph)) / (iters * replays))
            active.append(float((~(run.margin_min <= 0)).float().mean()))
        t_f.sort()
        t_s.sort()
        out = {"model": name, "batch": 100, "reps": reps, "iters_per_window": iters * replays,
               "forward_ms": round(t_f[reps // 2], 4), "forward_ms_spread": [round(t_f[0], 4), round(t_f[-1], 4)],
               "square_iter_ms": round(t_s[reps // 2], 4), "square_iter_ms_spread": [round(t_s[0], 4), round(t_s[-1], 4)],
               "active_at_window_end": round(sum(active) / len(active), 3)}
        out["square_over_forward"] = round(out["square_iter_ms"] / out["forward_ms"], 4)
        out["square_extra_us"] = round(1e3 * (out["square_iter_ms"] - out["forward_ms"]), 1)
        print("%s: eval forward %.4f ms [%.4f, %.4f], Square iteration %.4f ms [%.4f, %.4f] (x%.3f, +%.1f us); %.0f %% of the samples still "
              "active after %d iterations" % (name, out["forward_ms"], t_f[0], t_f[-1], out["square_iter_ms"], t_s[0], t_s[-1],
                                              out["square_over_forward"], out["square_extra_us"], 100 * out["active_at_window_end"],
                                              iters * replays), flush=True)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
