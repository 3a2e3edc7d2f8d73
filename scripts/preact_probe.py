#!/usr/bin/env python3
"""The AWP workload on PreActResNet18_EE_BPDA_3 (batch 100, 3x64x64, train mode as experiments_tiny_awp.py runs its attack loop): time and
kernel launches of one PGD iteration and of one whole AWP step (PGD-10 + proxy step + robust step, eeadv.trainer.awp_train_batch), with the
fused block boundary (ee_bn_sum_act_*) and with EEADV_STOCK_GLUE=preact (add + bn_act).

Times: graph replay as the driver runs it (EEADV_GRAPH=1), CUDA events, median of `reps`.  Launches: the same work run eagerly
(EEADV_GRAPH=0) under torch.profiler, device kernels counted - a replayed graph issues the same kernels.

    python scripts/preact_probe.py [reps]       -> one JSON line per variant, then a summary line
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


def child(reps):
    sys.path[:0] = [PKG, os.path.join(PKG, "AWP", "Tiny_imagenet")]
    import torch
    import models_tiny_awp as Z
    import utils.attacks as A
    from eeadv import trainer

    class Args:
        method_name, random, epsilon, num_steps_1, step_size_1, awp_warmup = "EE_AT_AWP", True, 16 / 255, 10, 2 / 255, 0

    kw = dict(dataset="Tiny-ImageNet", cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0)
    torch.manual_seed(0)
    net, proxy = Z.PreActResNet18_EE_BPDA_3(**kw).cuda().train(), Z.PreActResNet18_EE_BPDA_3(**kw).cuda()
    opt = trainer.make_sgd(net.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4)
    adv = Z.AdvWeightPerturb(model=net, proxy=proxy, proxy_optim=trainer.make_sgd(proxy.parameters(), lr=0.01), gamma=0.005)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(100, 3, 64, 64, generator=g).cuda()
    y = torch.randint(0, 200, (100,), generator=g).cuda()
    pgd = lambda k: A.PGD(net, Args, x, y, k, Args.step_size_1)
    step = lambda: trainer.awp_train_batch(net, adv, trainer.Criterion(), opt, Args, x, y, 0, x.device)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    def launches(fn):
        fn()
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                   and "Memset" not in e.name)

    out = {"glue": os.environ.get("EEADV_STOCK_GLUE", "") or "fused"}
    if os.environ.get("EEADV_GRAPH") == "0":
        out["launches_pgd1"] = launches(lambda: pgd(1))
        out["launches_pgd10"] = launches(lambda: pgd(10))
        out["launches_awp_step"] = launches(step)
    else:
        out["ms_pgd10"] = timed(lambda: pgd(10))
        out["ms_pgd_iter"] = out["ms_pgd10"] / 10
        out["ms_awp_step"] = timed(step)
    print(json.dumps(out), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rows = {}
    for glue in ("", "preact"):
        for graph in ("1", "0"):
            env = dict(os.environ, EEADV_STOCK_GLUE=glue, EEADV_GRAPH=graph, PREACT_PROBE_CHILD=str(reps))
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                raise SystemExit("probe child failed (glue=%r, graph=%s): exit %d" % (glue, graph, r.returncode))
            line = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(line), flush=True)
            rows.setdefault(line["glue"], {}).update(line)
    f, s = rows["fused"], rows["preact"]
    print(json.dumps({"summary": "fused vs EEADV_STOCK_GLUE=preact",
                      "pgd_iter_ms": [round(f["ms_pgd_iter"], 3), round(s["ms_pgd_iter"], 3)],
                      "awp_step_ms": [round(f["ms_awp_step"], 2), round(s["ms_awp_step"], 2)],
                      "launches_per_pgd_iter": [(f["launches_pgd10"] - f["launches_pgd1"]) / 9, (s["launches_pgd10"] - s["launches_pgd1"]) / 9],
                      "launches_awp_step": [f["launches_awp_step"], s["launches_awp_step"]]}))


if __name__ == "__main__":
    if os.environ.get("PREACT_PROBE_CHILD"):
        child(int(os.environ["PREACT_PROBE_CHILD"]))
    else:
        main()
