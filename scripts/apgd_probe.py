#!/usr/bin/env python3
"""What an APGD iteration costs next to a PGD iteration, and what APGD-T spends on samples that are already fooled.

Eval mode, batch 100 of synthetic 3x64x64 images, 200 classes, eps = 16/255, graph replay (EEADV_GRAPH=1), on `resnet18` and
`resnet18_EE_square` (the Tiny-ImageNet models).  Per-iteration time: CUDA events around whole attacks of 100 and of 20 iterations,
alternating PGD and APGD-CE, median of `reps`; (t100 - t20) / 80 leaves out what an attack pays once (start point, its forward/backward,
the initial state).  The APGD-T share: per run j of the targets, the fraction of the batch an earlier run (or the clean forward) had
already fooled; its mean over the runs (weighted by each run's time, and unweighted) is the share of APGD-T's time that went to
samples whose verdict was settled, because every run carries the whole batch (median of three timed runs per target).  The networks are untrained: labels are their own clean predictions, so clean accuracy is 100 %.

    python scripts/apgd_probe.py [reps]      -> a few text lines, then one JSON line per model
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
        runs = {"pgd": lambda k: A.PGD(m, Args, x, y, k, 2 / 255), "apgd_ce": lambda k: A.APGD(m, Args, x, y, k, "ce")}
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
            out[n + "_iter_ms"] = round((t100 - t20) / 80, 4)
            out[n + "_iter_ms_spread"] = [round((a - b) / 80, 4) for a, b in zip(sorted(ms[(n, 100)]), sorted(ms[(n, 20)]))][::max(reps - 1, 1)]
        out["apgd_over_pgd"] = round(out["apgd_ce_iter_ms"] / out["pgd_iter_ms"], 4)
        out["apgd_extra_us_per_iter"] = round(1e3 * (out["apgd_ce_iter_ms"] - out["pgd_iter_ms"]), 1)
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
