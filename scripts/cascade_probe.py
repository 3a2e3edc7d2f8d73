#!/usr/bin/env python3
"""What the survivor-only cascade saves over the whole-batch composite, on the bench model.

`resnet18_EE_square` (the Tiny-ImageNet model of bench.py), eval mode, batches of 100 synthetic 3x64x64 images, 200 classes, graph replay
(EEADV_GRAPH=1), the default budgets of a Tiny-ImageNet evaluation: 100 APGD iterations, 9 target classes, 100 FAB-T iterations per
target, 5000 Square queries.  For each epsilon: wall-clock time (device synchronised at both ends) of `--attack_method APGD+FAB+Square`
batch by batch (trainer.attack_for_validation) against `Cascade` (eeadv.cascade.evaluate) over the same batches, after one untimed
composite batch that captures the graphs both use.  The network is untrained and the labels are its own clean predictions, so the number
of samples that survive each stage - which is all the saving depends on - is NOT that of a trained model: at 16/255 nothing survives
APGD-CE and the cascade is APGD-CE alone, the small epsilon is there to show a run in which every stage has work.  `composite_robust`
counts correct predictions of ONE fresh forward of the composite's result; this model redraws its square at every forward, so that
count is not comparable with the cascade's flags ("never misclassified during the stage") and is printed for completeness only.

    python scripts/cascade_probe.py [n_batches] [eps255 ...]      -> one text line and one JSON line per epsilon
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


def main():
    os.environ["EEADV_GRAPH"] = "1"
    sys.path[:0] = [PKG]
    import torch
    from eeadv import cascade, models as M, trainer

    if not torch.cuda.is_available():
        raise SystemExit("cascade_probe: needs a ROCm device (a time taken on the host says nothing)")
    n_batches = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    eps255 = [float(v) for v in sys.argv[2:]] or [16.0, 0.25]
    dev = torch.device("cuda", 0)
    B, n_class, num_steps = 100, 200, 100

    class Args:
        random, method_name, attack_method, square_queries, fab_iters = True, "AT", "APGD+FAB+Square", 5000, 100

    torch.manual_seed(0)
    m = M.make_resnet_ee(18, "tiny", True, cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                         type_canny="CannyFilter_step125_1", epsilon=16 / 255, n_queries=1).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(n_batches):
        x = torch.rand(B, 3, 64, 64, generator=g).to(dev)
        with torch.no_grad():
            batches.append((x, m(x).argmax(1)))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for e in eps255:
        Args.epsilon = e / 255
        trainer.attack_for_validation(m, Args, *batches[0], dev, num_steps, None, n_class)  # captures (the graphs are keyed by epsilon)

        def composite():
            left = 0
            for x, y in batches:
                xa = trainer.attack_for_validation(m, Args, x, y, dev, num_steps, None, n_class)
                with torch.no_grad():
                    left += int((m(xa).argmax(1) == y).sum())
            return left

        t_comp, left = wall(composite)
        t_casc, res = wall(lambda: cascade.evaluate(m, Args, batches, n_class, num_steps=num_steps))
        out = {"model": "resnet18_EE_square", "batch": B, "n": res.n, "eps255": e, "composite_s": round(t_comp, 3), "cascade_s": round(t_casc, 3),
               "speedup": round(t_comp / t_casc, 2), "composite_robust": left, "clean_correct": res.clean_correct, "stages": res.stage_names,
               "rows_attacked": res.rows_attacked, "batches_attacked": res.batches_attacked, "robust_after": res.robust_after}
        print("eps %g/255, %d samples: APGD+FAB+Square %.2f s (%.2f s per batch), Cascade %.2f s (x%.1f); rows attacked per stage %s of %d clean-correct"
              % (e, res.n, t_comp, t_comp / n_batches, t_casc, t_comp / t_casc, res.rows_attacked, res.clean_correct))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
