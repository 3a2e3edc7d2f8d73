#!/usr/bin/env python3
"""What an APGD iteration costs next to a PGD iteration, and what APGD-T spends on samples that are already fooled.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, eps = 16/255, graph replay (EEADV_GRAPH=1), on `resnet18` and
`resnet18_EE_square` (the Tiny-ImageNet models).  Per-iteration time: CUDA events around whole attacks of 100 and of 20 iterations,
alternating PGD and APGD-CE, median of `reps`; (t100 - t20) / 80 leaves out what an attack pays once (start point, its forward/backward,
the initial state).  The APGD-T share: per run j of the targets, the fraction of the batch an earlier run (or the clean forward) had
already fooled; its mean over the runs (weighted by each run's time, and unweighted) is the share of APGD-T's time that went to
samples whose verdict was settled, because every run carries the whole batch (median of three timed runs per target).  The networks are untrained: labels are their own clean predictions, so clean accuracy is 100 %.

--restarts measures, on `resnet18` only and in place of the APGD-T part, an APGD-CE run of 2 restarts beside the
others - its time per iteration is (t100 - t20) / 160, the same graph replayed twice as often - and the two launches a restart adds, alone:
the start launch (100 rows of 12288 elements, the kernel's own draw, Linf and L2, both paths) and the merge launch (every row copied, and
none).

    python scripts/apgd_probe.py [reps] [--restarts]     -> a few text lines, then one JSON line per model
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
    from eeadv import models as M, ops

    if not torch.cuda.is_available():
        raise SystemExit("apgd_probe: needs a ROCm device (a time taken on the host says nothing)")
    argv = sys.argv[1:]
    restarts = "--restarts" in argv
    if restarts:
        argv.remove("--restarts")
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
            y = m(x).argmax(1)
        runs = {"pgd": lambda k: A.PGD(m, Args, x, y, k, 2 / 255), "apgd_ce": lambda k: A.APGD(m, Args, x, y, k, "ce")}
        if restarts:
            runs["apgd_ce_r2"] = lambda k: A.APGD(m, Args, x, y, k, "ce", n_restarts=2, seed=1)
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
            per = 160 if n == "apgd_ce_r2" else 80
            out[n + "_iter_ms"] = round((t100 - t20) / per, 4)
            out[n + "_iter_ms_spread"] = [round((a - b) / per, 4) for a, b in zip(sorted(ms[(n, 100)]), sorted(ms[(n, 20)]))][::max(reps - 1, 1)]
        out["apgd_over_pgd"] = round(out["apgd_ce_iter_ms"] / out["pgd_iter_ms"], 4)
        out["apgd_extra_us_per_iter"] = round(1e3 * (out["apgd_ce_iter_ms"] - out["pgd_iter_ms"]), 1)
        if restarts:
            xs_ = torch.empty_like(x)
            for metric in ("Linf", "L2"):
                for path in ("resident", "streaming"):
                    launch = lambda: [ops.apgd_start_(xs_, x, eps, metric, seed=1, path=path) for _ in range(50)]
                    launch()
                    torch.cuda.synchronize()
                    out["start_%s_%s_us" % (metric.lower(), path)] = round(1e3 * median([timed(launch) for _ in range(reps)]) / 50, 2)
            rob_all, loss_all = torch.ones(100, dtype=torch.int32, device=dev), torch.zeros(100, device=dev)
            loss_run = torch.ones(100, device=dev)
            for what, flag in (("copy", 0), ("idle", 1)):  # first = 1 with every row fooled copies every row; with none it copies nothing
                rob_run = torch.full((100,), flag, dtype=torch.int32, device=dev)
                launch = lambda: [ops.apgd_merge_(xs_, rob_all, loss_all, x, rob_run, loss_run, True) for _ in range(50)]
                launch()
                torch.cuda.synchronize()
                out["merge_%s_us" % what] = round(1e3 * median([timed(launch) for _ in range(reps)]) / 50, 2)
            out["apgd_r2_over_r1_iter"] = round(out["apgd_ce_r2_iter_ms"] / out["apgd_ce_iter_ms"], 4)
            out["apgd_r2_once_ms"] = round(out["apgd_ce_r2_ms_100"] - 200 * out["apgd_ce_r2_iter_ms"], 3)  # what a 2-restart run pays once
            out["apgd_r1_once_ms"] = round(out["apgd_ce_ms_100"] - 100 * out["apgd_ce_iter_ms"], 3)
            print("%s: APGD-CE with 2 restarts %.4f ms/iter (x%.4f of one run's %.4f, spread %s); start launch Linf %.1f / %.1f us, L2 %.1f / %.1f us "
                  "(resident / streaming); merge launch %.1f us copying every row, %.1f us copying none; paid once per call: %.3f ms with 2 "
                  "restarts, %.3f ms with one" % (name, out["apgd_ce_r2_iter_ms"], out["apgd_r2_over_r1_iter"], out["apgd_ce_iter_ms"],
                                                  out["apgd_ce_iter_ms_spread"], out["start_linf_resident_us"], out["start_linf_streaming_us"],
                                                  out["start_l2_resident_us"], out["start_l2_streaming_us"], out["merge_copy_us"],
                                                  out["merge_idle_us"], out["apgd_r2_once_ms"], out["apgd_r1_once_ms"]), flush=True)
            print(json.dumps(out), flush=True)
            continue
        # APGD-T, run by run, as utils.attacks.APGD_T does it (the flags are read on the host here, which the attack itself never does)
        n_t, k = 9, 20
        with torch.no_grad():
            order = ops.topk(m(x).float().contiguous(), None, n_t + 1)[0]
        A.APGD(m, Args, x, y, k, "dlr_t", order[:, 1].contiguous())  # untimed: captures the dlr_t graph and warms it up
        torch.cuda.synchronize()
        robust = torch.ones(100, dtype=torch.bool, device=dev)
        settled, t_runs, t_all = [], [], []
        for j in range(1, n_t + 1):
            settled.append(1.0 - float(robust.float().mean()))
            tj, res = [], []
            for _ in range(3):  # the flags of the first run count (each run draws its own start), the time is the median of three
                res.append(None)
                tj.append(timed(lambda: res.__setitem__(-1, A.APGD(m, Args, x, y, k, "dlr_t", order[:, j].contiguous()))))
            t_runs.append(median(tj))
            t_all.append([round(v, 3) for v in tj])
            robust &= res[0][1]
        out["apgd_t_ms_runs"] = t_all
        out["apgd_t_share_on_fooled_by_count"] = round(sum(settled) / len(settled), 4)
        out["apgd_t_targets"], out["apgd_t_iters"] = n_t, k
        out["apgd_t_fooled_before_run"] = [round(s, 3) for s in settled]
        out["apgd_t_robust_after"] = round(float(robust.float().mean()), 3)
        out["apgd_t_share_on_fooled"] = round(sum(s * t for s, t in zip(settled, t_runs)) / sum(t_runs), 4)
        out["apgd_t_ms_per_run"] = round(median(t_runs), 3)
        print("%s: PGD %.4f ms/iter, APGD-CE %.4f ms/iter (x%.3f, +%.1f us); APGD-T (%d targets x %d iterations): %.1f %% of its time on "
              "samples already fooled, %.1f %% robust at the end" % (name, out["pgd_iter_ms"], out["apgd_ce_iter_ms"], out["apgd_over_pgd"],
                                                                    out["apgd_extra_us_per_iter"], n_t, k, 100 * out["apgd_t_share_on_fooled"],
                                                                    100 * out["apgd_t_robust_after"]), flush=True)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
