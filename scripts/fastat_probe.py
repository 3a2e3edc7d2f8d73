#!/usr/bin/env python3
"""What a step of fast adversarial training costs at the phase-1 shape: `resnet50` on synthetic 3 x 128 x 128 batches,
the largest batch <= 512 that fits, train mode, fp32.

The captured step (trainer.FastAtStep with EEADV_GRAPH=1: one graph replay per step, the learning rate changed before every step) against
the eager one (trainer.fast_at_step on the same tree: the same launches issued from Python), un-profiled: CUDA events around runs of `n`
steps, alternating the two, median of `reps` runs, after the warm-up each needs (two eager steps and the capture).  Launches per step are
counted apart from the timing, with torch's profiler around ONE eager step.  Writes images/s, milliseconds per step and launches per
step to profiles/fastat_probe.txt.

    python scripts/fastat_probe.py [reps] [n]     (defaults 3 and 4: the recorded run)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


def main():
    sys.path[:0] = [PKG, os.path.join(PKG, "ImageNet")]
    import torch
    import models_imagenet as zoo
    from eeadv import runtime, trainer

    if not torch.cuda.is_available():
        raise SystemExit("fastat_probe: needs a ROCm device (a time taken on the host says nothing)")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    dev = torch.device("cuda", 0)
    runtime.use_shipped_miopen_db()
    eps, alpha, S = 4 / 255, 5 / 255, 128

    def build(B, graph):
        os.environ["EEADV_GRAPH"] = "1" if graph else "0"
        torch.manual_seed(0)
        m = zoo.resnet50(num_classes=1000)
        m.avgpool = torch.nn.AdaptiveAvgPool2d(1)
        m = m.to(dev).train()
        opt = trainer.make_fast_sgd(m, 0.1, momentum=0.9, weight_decay=1e-4)
        noise = torch.zeros(B, 3, S, S, device=dev)
        return trainer.FastAtStep(m, trainer.Criterion(), opt, noise, alpha, eps, random_init=True, seed=1)

    def run(step, x, y, k, graph):
        os.environ["EEADV_GRAPH"] = "1" if graph else "0"
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(k):
            step.set_lr(0.1 + 0.01 * i)
            step(x, y)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    lines = []
    for B in (512, 384, 256, 128, 64):
        try:
            g = torch.Generator().manual_seed(B)
            x, y = torch.rand(B, 3, S, S, generator=g).to(dev), torch.randint(0, 1000, (B,), generator=g).to(dev)
            sg, se = build(B, True), build(B, False)
            run(sg, x, y, 3, True)  # two eager steps, then the capture and its first replay
            run(se, x, y, 2, False)
        except torch.OutOfMemoryError:
            sg = se = None
            torch.cuda.empty_cache()
            lines.append("batch %d does not fit" % B)
            continue
        tg, te = [], []
        for _ in range(reps):
            tg.append(run(sg, x, y, n, True))
            te.append(run(se, x, y, n, False))
        mg, me = sorted(tg)[reps // 2], sorted(te)[reps // 2]
        launches = "n/a"
        try:
            from torch.profiler import ProfilerActivity, profile
            os.environ["EEADV_GRAPH"] = "0"
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                se(x, y)
                torch.cuda.synchronize()
            launches = str(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))
        except Exception as exc:  # noqa: BLE001 - the count is a side note; the times above stand without it
            launches = "n/a (%s)" % type(exc).__name__
        lines += ["%s, resnet50, batch %d x 3 x %d x %d, fp32, train mode, %d captures" % (torch.cuda.get_device_name(0), B, S, S, sg.captures),
                  "captured step (one replay): %.2f ms per step, %.0f images/s  (runs: %s)" % (mg, 1000 * B / mg, " ".join("%.2f" % t for t in tg)),
                  "eager step (fast_at_step):  %.2f ms per step, %.0f images/s  (runs: %s)" % (me, 1000 * B / me, " ".join("%.2f" % t for t in te)),
                  "device launches in one eager step: %s" % launches]
        break
    out = os.path.join(ROOT, "profiles", "fastat_probe.txt")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
